"""dense_predict_kernel (through ochip_dense_link's slot rows) and the two triangulation kernels (ochip_dense_triangulate),
raw through the C ABI, against the long-double reference of tests/dense_kernel_fixtures.py: which cameras were chosen, in
which order and which passed the image test, exactly; which tracks get a point, exactly, and the points within
C_TRI 2^-53 kappa scale.  Both routes: the LDS-staged one and the one of surveys above 2 048 images
(OCHIP_TEST_HOOKS=dense_predict_unstaged).  tests/test_dense_kernel_fixtures.py holds the fixtures themselves on the CPU.

Measured on an MI355X: DENSE_TRI_RATIOS worst 3.73 of the bound at C = 1 (track "tri2/bulk11", both routes) - the figure the
fp64 numpy restatement gives on the CPU, to the digit; C_TRI = 8."""
import ctypes as C
import json

import numpy as np
import pytest

from opencalibration_amd import capi
from oracle import pyoracle
import dense_kernel_fixtures as F

pytestmark = pytest.mark.gpu

OCHIP_EINVAL, OCHIP_ESTATE = -1, -5
HOOKS = (None, "dense_predict_unstaged")


class _Index:
    """one ochip_dense_index over per-image (locations, descriptors)"""

    def __init__(self, ctx, features):
        self.ctx, self.L = ctx, ctx.L
        L, vp = self.L, C.c_void_p
        L.ochip_dense_index_create.argtypes = [vp, C.c_uint32] + [vp] * 7 + [C.c_double, C.POINTER(vp)]
        L.ochip_dense_index_destroy.argtypes = [vp]
        L.ochip_dense_index_destroy.restype = None
        L.ochip_dense_link.argtypes = [vp, vp, vp, vp, C.c_double, C.c_uint32, C.c_uint32, C.c_double, C.c_double, vp, vp, vp]
        L.ochip_dense_triangulate.argtypes = [vp, vp, C.c_uint32, vp, vp, C.c_double, vp, vp]
        self.ix = ix = F.index_arrays(features)
        self.h = vp()
        rc = L.ochip_dense_index_create(ctx.h, ix["n_images"], ix["feat_off"].ctypes.data, ix["desc"].ctypes.data, ix["loc"].ctypes.data,
                                        ix["cell_off"].ctypes.data, ix["cell_start"].ctypes.data, ix["grid2"].ctypes.data,
                                        ix["origin2"].ctypes.data, F.CELL, C.byref(self.h))
        assert rc == 0, L.ochip_last_error(ctx.h)

    def link(self, cams17, hits):
        total = self.ix["total"]
        root, counts, slots = np.zeros(total, np.uint32), np.zeros(2, np.uint64), np.zeros((total, F.DENSE_K), np.uint32)
        cams17, hits = np.ascontiguousarray(cams17, np.float64), np.ascontiguousarray(hits, np.float64)
        rc = self.L.ochip_dense_link(self.h, cams17.ctypes.data, self.ix["id_of_pos"].ctypes.data, hits.ctypes.data, F.RADIUS, F.DENSE_K - 1,
                                     F.DESCRIPTOR_BITS, F.RATIO, F.MAX_ABS, root.ctypes.data, counts.ctypes.data, slots.ctypes.data)
        assert rc == 0, self.L.ochip_last_error(self.ctx.h)
        return root, counts, slots

    def triangulate(self, cam_q, start, member):
        """(rc, points [k][3], valid [k])"""
        k = len(start) - 1
        cam_q = np.ascontiguousarray(cam_q, np.float64)
        points, valid = np.full((max(k, 1), 3), np.nan), np.full(max(k, 1), 7, np.uint8)
        rc = self.L.ochip_dense_triangulate(self.h, cam_q.ctypes.data, k, start.ctypes.data, member.ctypes.data, F.MAX_REPROJECTION,
                                            points.ctypes.data, valid.ctypes.data)
        return rc, points[:k], valid[:k]

    def close(self):
        self.L.ochip_dense_index_destroy(self.h)


class _Worst:
    def __init__(self):
        self.ratio, self.where = 0.0, None

    def add(self, where, ratio):
        if ratio > self.ratio:
            self.ratio, self.where = float(ratio), where

    def line(self, checked):
        return json.dumps({"worst_ratio_of_bound": float("%.3g" % (self.ratio / F.C_TRI)), "worst_ratio_at_C_1": float("%.3g" % self.ratio),
                           "C_TRI": F.C_TRI, "track": self.where, "results_checked": checked})


def _context(hook, monkeypatch):
    if hook:
        monkeypatch.setenv("OCHIP_TEST_HOOKS", hook)
    return capi.Context(0)


@pytest.mark.parametrize("hook", HOOKS)
@pytest.mark.parametrize("family", ["counts", "far", "distortion", "ties", "clamp"])
def test_predict_slot_rows_against_long_double(family, hook, monkeypatch):
    """the slot rows name the twin in every in-image camera among the 11 smallest (d^2, index), the source skipped, in that
    order; the counts are the candidates'; the roots a plain union-find's"""
    ctx = _context(hook, monkeypatch)
    for s in F.predict_scenes():
        if s["family"] != family:
            continue
        index = _Index(ctx, s["features"])
        hits, exp_slots = F.by_position(s, index.ix)
        root, counts, slots = index.link(F.cams17(s["pos"], s["q"], s["models"]), hits)
        wrong = np.nonzero((slots != exp_slots).any(1))[0]
        assert len(wrong) == 0, "%s: %d rows differ, first at position %d (measurement %d): %s, expected %s" % (
            s["name"], len(wrong), wrong[0], index.ix["id_of_pos"][wrong[0]], slots[wrong[0]], exp_slots[wrong[0]])
        assert (int(counts[0]), int(counts[1])) == (s["exp_queries"], s["exp_queries"]), s["name"]
        assert np.array_equal(root, s["exp_root"]), s["name"]
        index.close()
    ctx.close()


def test_triangulate_against_long_double(monkeypatch):
    """every call of every scene on both routes: valid exactly, the points within the bound; one line with the worst ratio"""
    scenes = F.tri_scenes(pyoracle.image_to_3d)
    worst, problems, checked = _Worst(), [], 0
    for hook in HOOKS:
        if hook:
            monkeypatch.setenv("OCHIP_TEST_HOOKS", hook)
        ctx = capi.Context(0)
        for s in scenes:
            cams = s["cams"]
            index = _Index(ctx, s["features"])
            root, counts, _ = index.link(F.cams17(cams["pos"], cams["q"], cams["models"]), np.full((s["total"], 3), np.nan))
            assert (root == F.NONE).all() and not counts.any(), s["name"]           # no hits: nothing is matched
            for call, numbers in s["calls"].items():
                start, member = F.call_arrays(s, numbers)
                rc, points, valid = index.triangulate(cams["q"], start, member)
                assert rc == 0, (s["name"], call, ctx.L.ochip_last_error(ctx.h))
                assert set(valid.tolist()) <= {0, 1}, (s["name"], call)
                for k, i in enumerate(numbers):
                    t = s["tracks"][i]
                    problem, ratio = F.check_track(t, valid[k], points[k])
                    checked += 1
                    if problem:
                        problems.append("%s, call %s, route %s: %s" % (s["name"], call, hook or "staged", problem))
                    if ratio is not None:
                        worst.add("%s (call %s, %s)" % (t["name"], call, hook or "staged"), ratio)
            index.close()
        ctx.close()
    print("DENSE_TRI_RATIOS", worst.line(checked))
    assert checked > 1000 and problems == [], problems[:10]
    assert worst.ratio <= F.C_TRI


def test_triangulate_refusals_leave_the_index_working():
    s = F.tri_scenes(pyoracle.image_to_3d)[1]
    cams = s["cams"]
    ctx = capi.Context(0)
    index = _Index(ctx, s["features"])
    numbers = s["calls"]["all"][:12]
    start, member = F.call_arrays(s, numbers)
    rc, _, _ = index.triangulate(cams["q"], start, member)
    assert rc == OCHIP_ESTATE and b"ochip_dense_link has not run" in ctx.L.ochip_last_error(ctx.h)      # triangulate before link
    assert index.triangulate(cams["q"], np.zeros(1, np.uint32), np.zeros(0, np.uint32))[0] == 0              # (no tracks: nothing to do)
    index.link(F.cams17(cams["pos"], cams["q"], cams["models"]), np.full((s["total"], 3), np.nan))
    beyond = member.copy()
    beyond[len(beyond) // 2] = s["total"]
    assert index.triangulate(cams["q"], start, beyond)[0] == OCHIP_EINVAL                                   # a member that is no measurement
    beyond[len(beyond) // 2] = 0xFFFFFFFF
    assert index.triangulate(cams["q"], start, beyond)[0] == OCHIP_EINVAL
    descending = start.copy()
    descending[3], descending[4] = start[4], start[3]
    assert index.triangulate(cams["q"], descending, member)[0] == OCHIP_EINVAL                              # track_start must ascend
    rc, points, valid = index.triangulate(cams["q"], start, member)                                         # ... and the index still works
    assert rc == 0
    assert [F.check_track(s["tracks"][i], valid[k], points[k])[0] for k, i in enumerate(numbers)] == [None] * len(numbers)
    assert valid.sum() >= 6
    index.close()
    ctx.close()

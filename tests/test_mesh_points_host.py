"""The flat locate table's CPU route (csrc/mesh_locate.hpp run by host/mesh_points.cpp) against the
existing host route (countPointsPerTriangle / TriangleLocator of host/refine_mesh.cpp) and the oracle's restatement, and the
DENSE_MESH_RELAX state against pipeline.cpp:844-924 written out over the oracle's pieces.  Bit for bit; no device."""
import numpy as np
import pytest

import mesh_points_fixtures as F
from opencalibration_amd import host
from oracle import pyoracle
from relax_fixtures import MODEL_600


@pytest.mark.parametrize("name", F.MESHES)
def test_flat_count_equals_the_host_route_and_the_oracle(name):
    s = F.mesh(name)
    a = s.arrays()
    rx = pyoracle.RxMesh(a["vertices"], a["edges"])
    for key, clouds in F.clouds_for(s).items():
        s.set_clouds(clouds)
        old, flat = s.count_points_per_triangle(), s.count_points_per_triangle(flat=True)
        assert F.same_rows(flat, old), key
        if clouds:
            assert F.same_rows(flat, rx.count_points_per_triangle(clouds)), key
        if key == "two":
            assert len(flat[0]) > 1 and flat[1].sum() > 700
            s.set_clouds(clouds[::-1])              # the other concatenation order: other rows first
            swapped = s.count_points_per_triangle(flat=True)
            assert F.same_rows(swapped, s.count_points_per_triangle()) and not np.array_equal(swapped[0], flat[0])
        if key == "empty":
            assert len(flat[0]) == 0
        if key == "one":
            assert list(flat[1]) == [1] and flat[2][0] == 0.0
        if key == "one_and_two":
            assert sorted(flat[1]) == [1, 2] and flat[2][list(flat[1]).index(1)] == 0.0


@pytest.mark.parametrize("name", F.MESHES)
def test_flat_locate_equals_the_locator(name):
    s = F.mesh(name)
    q = F.locate_cases(s)
    old, flat = s.locate(q), s.locate(q, flat=True)
    assert np.array_equal(old, flat)
    assert (old[-14:, 0] == F.NONE).all()                      # the points outside and the far ones: no triangle
    assert (old[:-14, 0] != F.NONE).all()                      # vertices, midpoints, centroids, the centre: inside
    if name == "minimal":
        # the centre of the square is equidistant from both centroids: the walk starts from - and ends in - the lower index
        table = s.locate_table()
        centre = q[-15]
        d = (table["cx"] - centre[0]) ** 2 + (table["cy"] - centre[1]) ** 2
        first = int(np.flatnonzero(d == d.min())[0])
        assert np.sum(d == d.min()) > 1
        tri_of_first = s.locate(np.array([[table["cx"][first], table["cy"][first]]]))[0]
        assert sorted(old[-15]) == sorted(tri_of_first)


def test_locate_table_is_consistent():
    """What the device entry checks before it launches holds for the tables the host builds."""
    for name in F.MESHES:
        t = F.mesh(name).locate_table()
        T = len(t["vertex_xy"])
        assert T == 3 * len(F.triangles(F.mesh(name)))            # a triangle is located under each of its edges
        assert len(t["start"]) == t["nx"] ** 2 + 1 and t["start"][0] == 0 and t["start"][-1] == T
        assert (np.diff(t["start"].astype(np.int64)) >= 0).all() and sorted(t["items"]) == list(range(T))
        nb = t["neighbours"]
        assert ((nb < T) | (nb == 0xFFFFFFFF)).all()
        n = t["plane"][:, 3:]
        assert np.allclose(np.sum(n * n, axis=1), 1.0, rtol=0, atol=1e-12)


@pytest.mark.parametrize("max_steps", [0, 1, 2])
def test_exhausted_walks_fall_back_to_the_exhaustive_scan(max_steps):
    """A walk that runs out of steps is resolved by brute force on the host.  For points strictly inside a triangle the
    scan finds the same triangle - under the first of its three names in edge order, where the walk names it by the edge it
    entered through, so triangles are compared as vertex sets and counts per vertex set."""
    s = F.mesh("refined1")
    pts, owner = F.inside_points(s, 600)
    got, full = s.locate(pts, max_steps=max_steps), s.locate(pts, max_steps=100)
    assert np.array_equal(full, s.locate(pts))
    assert F.vertex_sets(got) == F.vertex_sets(full) == owner
    xyz = np.concatenate([pts, np.sin(pts[:, :1])], axis=1)
    few, many = host.PointCounter(xyz, max_steps=max_steps), host.PointCounter(xyz, max_steps=100)
    rows_few, rows_many = few.count(s), many.count(s)
    assert many.exhausted == 0 and few.exhausted > (0 if max_steps else len(pts) - 1)
    s.set_clouds([xyz])
    assert F.same_rows(rows_many, s.count_points_per_triangle())
    assert F.counts_by_triangle(rows_few) == F.counts_by_triangle(rows_many)
    assert sum(rows_few[1]) == len(pts)
    if max_steps == 0:
        # every point went through the scan: the rows are the scan's triangles in first-point order, sums redone on the host
        first = []
        for t in (tuple(int(x) for x in r) for r in got):
            if t not in first:
                first.append(t)
        assert [tuple(int(x) for x in r) for r in rows_few[0]] == first


@pytest.mark.parametrize("name", ["early", "capped"])
def test_dense_mesh_relax_equals_the_oracle(name):
    pos, ground, cloud = F.relax_scene(name)
    s = F.scene_surface(pos, ground, cloud)
    a = s.arrays()
    rx = pyoracle.RxMesh(a["vertices"], a["edges"])
    olog = F.oracle_dense_mesh_relax(rx, [cloud], pos, MODEL_600, 40)
    if name == "early":      # ends because a run created nothing, before the cap
        assert 3 < len(olog) < 21 and olog[-1]["created"] == 0 and all(r["created"] > 0 for r in olog[:-1])
    else:                    # still creating in run 20: the cap ends it
        assert len(olog) == 21 and olog[-1]["run"] == 20 and all(r["created"] > 0 for r in olog)
    g = F.scene_graph(pos)
    out, log = g.dense_mesh_relax(s)
    assert out is s and F.same_log(log, olog), (log, olog)
    assert F.same_mesh(s, rx)
    assert len(s.clouds()) == 1 and np.array_equal(s.clouds()[0], cloud)       # the state leaves the cloud alone
    g.close()


def test_dense_mesh_relax_exits():
    pos, ground, cloud = F.relax_scene("early")
    g = F.scene_graph(pos)
    # an empty surface list: the state is left at once
    s, log = g.dense_mesh_relax(host.Surface())
    assert len(log) == 1 and log[0]["created"] == 0 and log[0]["vertices"] == 0 and len(s.arrays()["vertices"]) == 0
    # a surface without a mesh: nothing to refine
    cloud_only = host.Surface().set_clouds([cloud])
    s, log = g.dense_mesh_relax(cloud_only)
    assert len(log) == 1 and log[0]["created"] == 0 and len(s.arrays()["vertices"]) == 0 and len(s.clouds()[0]) == len(cloud)
    # max_steps cuts the loop
    s, log = g.dense_mesh_relax(F.scene_surface(pos, ground, cloud), max_steps=2)
    assert [r["run"] for r in log] == [0, 1] and log[1]["created"] > 0
    g.close()
    # no usable camera: gsd = 0.01, reduced gsd = 0, as the oracle's restatement with no camera
    nowhere = pos.copy()
    nowhere[:, 2] = np.nan
    g = F.scene_graph(nowhere)
    s = F.scene_surface(pos, ground, cloud)
    a = s.arrays()
    rx = pyoracle.RxMesh(a["vertices"], a["edges"])
    olog = F.oracle_dense_mesh_relax(rx, [cloud], [], MODEL_600, 40)
    s, log = g.dense_mesh_relax(s)
    assert log[0]["gsd"] == 0.01 and log[0]["reduced_gsd"] == 0.0
    assert F.same_log(log, olog) and F.same_mesh(s, rx)
    g.close()

"""Points per triangle on the device (csrc/mesh_points.hip) against the CPU route of the same
library, which runs the same header (csrc/mesh_locate.hpp) in host loops and is itself held against the existing host route
and the oracle by test_mesh_points_host.py.  Bit for bit: triangle ids, row order, counts, variances, located triangles,
meshes."""
import numpy as np
import pytest

import mesh_points_fixtures as F
from opencalibration_amd import capi, host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", F.MESHES)
def test_device_count_and_locate_equal_the_cpu_route(ctx, name):
    s = F.mesh(name)
    for key, clouds in F.clouds_for(s).items():
        s.set_clouds(clouds)
        assert F.same_rows(s.count_points_per_triangle(ctx=ctx), s.count_points_per_triangle(flat=True)), key
    q = F.locate_cases(s)
    assert np.array_equal(s.locate(q, ctx=ctx), s.locate(q, flat=True))
    assert len(s.locate(np.zeros((0, 2)), ctx=ctx)) == 0


@pytest.mark.parametrize("max_steps", [0, 1, 2])
def test_device_exhausted_walks_equal_the_cpu_route(ctx, max_steps):
    s = F.mesh("refined1")
    pts, owner = F.inside_points(s, 600)
    assert np.array_equal(s.locate(pts, ctx=ctx, max_steps=max_steps), s.locate(pts, max_steps=max_steps))
    xyz = np.concatenate([pts, np.sin(pts[:, :1])], axis=1)
    dev, cpu = host.PointCounter(xyz, ctx=ctx, max_steps=max_steps), host.PointCounter(xyz, max_steps=max_steps)
    assert F.same_rows(dev.count(s), cpu.count(s)) and dev.exhausted == cpu.exhausted > 0
    dev.close()


def _cloud_in(surface, tri, n, seed, spread=0.2):
    """n points around the centroid of triangle tri (a sorted vertex triple), rolling heights.  Near its centroid a
    triangle is found under one name - the first of its three edges - so its points make one row and one segment."""
    rng = np.random.default_rng(seed)
    v = surface.arrays()["vertices"]
    w = rng.dirichlet([1.0, 1.0, 1.0], n) * spread + (1 - spread) / 3
    p = w @ v[list(tri)]
    p[:, 2] += 0.3 * np.sin(p[:, 0]) + rng.normal(0, 0.01, n)
    return p


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_one_triangle_at_wave_and_workgroup_boundaries(ctx, n):
    """A segment of 63, 64, 65 and 257 distances: a partial batch, exactly one, one and a lane, four and a lane."""
    s = F.mesh("grid3x3")
    s.set_clouds([_cloud_in(s, F.triangles(s)[3], n, n)])
    dev = s.count_points_per_triangle(ctx=ctx)
    assert F.same_rows(dev, s.count_points_per_triangle(flat=True)) and list(dev[1]) == [n]


def test_two_long_segments_on_the_minimal_mesh(ctx):
    """70 000 points in each of the minimal mesh's two triangles: segments longer than 65 535, the long sequential chains."""
    s = F.minimal_mesh()
    t0, t1 = F.triangles(s)
    a, b = _cloud_in(s, t0, 70000, 1), _cloud_in(s, t1, 70000, 2)
    pts = np.empty((140000, 3))
    pts[0::2], pts[1::2] = a, b
    s.set_clouds([pts])
    dev = s.count_points_per_triangle(ctx=ctx)
    assert F.same_rows(dev, s.count_points_per_triangle(flat=True))
    assert list(dev[1]) == [70000, 70000] and F.counts_by_triangle(dev) == {t0: 70000, t1: 70000}


def test_refined_mesh_outside_cloud_and_cloud_order(ctx):
    s = F.mesh("refined3")
    assert len(F.triangles(s)) > 100
    lo, hi = F.extent(s)
    rng = np.random.default_rng(3)
    xy = rng.uniform(lo - 2, hi + 2, (5000, 2))
    pts = np.concatenate([xy, (np.sin(xy[:, :1] / 5) + rng.normal(0, 0.05, (5000, 1)))], axis=1)
    s.set_clouds([pts])
    rows = s.count_points_per_triangle(ctx=ctx)
    assert F.same_rows(rows, s.count_points_per_triangle(flat=True)) and len(rows[0]) > 100
    # every point outside: no rows
    out = pts.copy()
    out[:, 0] += (hi[0] - lo[0]) + 10
    s.set_clouds([out])
    assert len(s.count_points_per_triangle(ctx=ctx)[0]) == 0
    # the cloud in two halves, in both orders: the same triangles with the same counts, in another order: a row sits where
    # its triangle first receives a point (and the sums run in the new point order)
    s.set_clouds([pts[:2500], pts[2500:]])
    ab = s.count_points_per_triangle(ctx=ctx)
    s.set_clouds([pts[2500:], pts[:2500]])
    ba = s.count_points_per_triangle(ctx=ctx)
    assert F.same_rows(ab, rows) and F.same_rows(ba, s.count_points_per_triangle(flat=True))
    key = lambda r: sorted((tuple(int(x) for x in t), int(c)) for t, c in zip(r[0], r[1]))
    assert key(ab) == key(ba) and not np.array_equal(ab[0], ba[0])


def test_one_handle_against_successive_meshes(ctx):
    """Nothing is carried from one count to the next: one counter over three meshes - before and after refinements - gives
    what fresh counters give, and the CPU route."""
    pos, ground, cloud = F.relax_scene("early")
    s = F.scene_surface(pos, ground, cloud)
    kept = host.PointCounter(cloud, ctx=ctx)
    for rnd in range(3):
        fresh, cpu = host.PointCounter(cloud, ctx=ctx), host.PointCounter(cloud)
        rows = kept.count(s)
        assert F.same_rows(rows, fresh.count(s)) and F.same_rows(rows, cpu.count(s)) and len(rows[0]) > 1
        fresh.close()
        assert s.refine_by_point_density(20, 1e-4, 2, min_triangle_size=0.5) > 0
    kept.close()


@pytest.mark.parametrize("name", ["early", "capped"])
def test_dense_mesh_relax_on_the_device_equals_the_cpu_route(ctx, name):
    pos, ground, cloud = F.relax_scene(name)
    g = F.scene_graph(pos)
    dev, log_dev = g.dense_mesh_relax(F.scene_surface(pos, ground, cloud), ctx=ctx)
    cpu, log_cpu = g.dense_mesh_relax(F.scene_surface(pos, ground, cloud))
    assert F.same_log(log_dev, log_cpu) and F.same_mesh(dev, cpu)
    assert len(log_dev) == (21 if name == "capped" else 7)
    g.close()


def test_refusals(ctx):
    s = F.mesh("refined0")
    table = s.locate_table()
    T = len(table["vertex_xy"])
    # n = 0 is valid
    none = capi.MeshPoints(ctx, np.zeros((0, 3)))
    r = none.count(table)
    assert r["count"].sum() == 0 and len(r["exhausted"]) == 0 and len(r["where"]) == 0
    none.close()
    pts = np.concatenate([F.inside_points(s, 50)[0], np.zeros((50, 1))], axis=1)
    m = capi.MeshPoints(ctx, pts)
    good = m.count(table)
    assert good["count"].sum() == 50 and (good["where"] < T).all()

    def broken(**change):
        t = dict(table)
        for k, f in change.items():
            t[k] = f(np.array(table[k]))
        return t

    def put(a, index, value):
        a[index] = value
        return a

    bad = {"neighbour": broken(neighbours=lambda a: put(a, (T // 2, 1), T)),
           "start not monotone": broken(start=lambda a: put(a, 1, a[-1] + 1) if len(a) > 2 else put(a, 0, 5)),
           "item": broken(items=lambda a: put(a, T - 1, T)),
           "start too short": broken(start=lambda a: a[:-1])}
    for what, t in bad.items():
        with pytest.raises(capi.OchipError, match="inconsistent table"):
            m.count(t)
    assert np.array_equal(m.count(table)["count"], good["count"])      # and the object still counts
    # a destroyed handle is refused, not followed
    handle = m.raw
    m.close()
    with pytest.raises(capi.OchipError, match="not a live"):
        m.count(table, handle=handle)

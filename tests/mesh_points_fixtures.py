"""Meshes, clouds, locate cases and the scenes of the DENSE_MESH_RELAX state shared by test_mesh_points_host.py (the flat
route on the CPU against the existing host route and the oracle) and test_gpu_mesh_points.py (the device route against the
flat CPU route).  Everything is compared bit for bit."""
import functools

import numpy as np

from opencalibration_amd import host
from oracle import pyoracle
from relax_fixtures import DOWN, MODEL_600, host_graph_from_edges

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def same_rows(a, b):
    """(tri, count, variance): ids, order, counts and the variances' float64 bit patterns."""
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2].dtype == np.float64 == b[2].dtype
            and np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64)))


def same_mesh(surface, other):
    """_same_mesh of test_refine_mesh.py for two surfaces or a surface and an oracle mesh."""
    a = surface.arrays()
    v, e = other.arrays() if isinstance(other, pyoracle.RxMesh) else (other.arrays()["vertices"], other.arrays()["edges"])
    return np.array_equal(a["vertices"].view(np.uint64), v.view(np.uint64)) and np.array_equal(a["edges"], e)


def minimal_mesh():
    return host.rebuild_mesh(np.array([[0, 0, 10], [10, 10, 10.0]]), minimal=True)


def grid_mesh(nx, ny):
    cams = np.array([[x * 20.0, y * 20.0, 50.0] for x in range(nx) for y in range(ny)])
    return host.rebuild_mesh(cams)


def refined_mesh(seed):
    """The loop of test_refinement_equals_the_oracle_restatement: four rounds of refine_by_point_density, heights moved."""
    rng = np.random.default_rng(seed)
    cams = np.array([[x, y, 50.0] for x in np.arange(0, 60 + 10 * seed, 20) for y in np.arange(0, 60, 20)], float)
    cams[:, :2] += rng.uniform(-2, 2, (len(cams), 2))
    s = host.rebuild_mesh(cams, minimal=(seed % 2 == 0))
    lo, hi = cams[:, :2].min(0) - 5, cams[:, :2].max(0) + 5
    for rnd in range(4):
        pts = np.concatenate([rng.uniform(lo, hi, (900, 2)), np.zeros((900, 1))], axis=1)
        pts[:, 2] = 1.5 * np.sin(pts[:, 0] / 7.0 + rnd) * np.cos(pts[:, 1] / 5.0) + rng.normal(0, 0.02, len(pts))
        s.set_clouds([pts[:400], pts[400:]])
        s.refine_by_point_density(20, 0.01, 2, min_triangle_size=1.0)
        a = s.arrays()
        s.set_heights(a["vertices"][:, 2] + rng.normal(0, 0.05, len(a["vertices"])))
    s.set_clouds([])
    return s


@functools.lru_cache(maxsize=None)
def mesh_arrays():
    """name -> (vertices, edges) of every mesh of the tests (built once; a test takes a fresh Surface from them)."""
    out = {"minimal": minimal_mesh(), "grid3x3": grid_mesh(3, 3), "grid4x3": grid_mesh(4, 3)}
    for seed in range(4):
        out["refined%d" % seed] = refined_mesh(seed)
    return {k: (s.arrays()["vertices"], s.arrays()["edges"]) for k, s in out.items()}


MESHES = ["minimal", "grid3x3", "grid4x3", "refined0", "refined1", "refined2", "refined3"]


def mesh(name):
    v, e = mesh_arrays()[name]
    return host.Surface().set(v, e)


def triangles(surface):
    """The mesh's triangles as sorted vertex triples."""
    tris = set()
    for s, d, border, o0, o1 in surface.arrays()["edges"]:
        for o in ([o0] if border else [o0, o1]):
            if o != NONE:
                tris.add(tuple(sorted((int(s), int(d), int(o)))))
    return sorted(tris)


def extent(surface):
    v = surface.arrays()["vertices"][:, :2]
    return v.min(0), v.max(0)


def clouds_for(surface, seed=5):
    """name -> list of clouds: two clouds of 400 and 500 points (so the concatenation order matters), none, one point, and
    a cloud that leaves one triangle exactly 1 point and another exactly 2 (the count > 1 rule)."""
    rng = np.random.default_rng(seed)
    lo, hi = extent(surface)
    pad = 0.05 * (hi - lo)
    xy = rng.uniform(lo - pad, hi + pad, (900, 2))
    z = 1.5 * np.sin(xy[:, 0] / 7.0) * np.cos(xy[:, 1] / 5.0) + rng.normal(0, 0.02, len(xy))
    pts = np.concatenate([xy, z[:, None]], axis=1)
    v = surface.arrays()["vertices"]
    tris = triangles(surface)
    c0, c1 = v[list(tris[0])], v[list(tris[-1])]
    w = np.array([[0.5, 0.3, 0.2], [0.2, 0.2, 0.6], [0.6, 0.3, 0.1]])
    few = np.concatenate([w[:1] @ c0, w[1:] @ c1]) + [0, 0, 0.25]
    return {"two": [pts[:400], pts[400:]], "empty": [], "one": [pts[7:8]], "one_and_two": [few]}


def locate_cases(surface):
    """Every vertex, edge midpoint and centroid; the centre of the mesh's bounding square (on the minimal mesh equidistant
    from both centroids: the lower index decides); points outside near each border; two far points for the ring search."""
    a = surface.arrays()
    v, e = a["vertices"][:, :2], a["edges"]
    mids = (v[e[:, 0].astype(int)] + v[e[:, 1].astype(int)]) / 2
    cents = np.array([v[list(t)].mean(0) for t in triangles(surface)])
    lo, hi = extent(surface)
    c, h = (lo + hi) / 2, (hi - lo) / 2
    outside = []
    for f in (-0.7, 0.0, 0.45):
        outside += [[lo[0] - 0.37, c[1] + f * h[1]], [hi[0] + 0.37, c[1] + f * h[1]], [c[0] + f * h[0], lo[1] - 0.37],
                    [c[0] + f * h[0], hi[1] + 0.37]]
    far = [[1e6, 0.0], [-1e6, -1e6]]
    return np.concatenate([v, mids, cents, [c], outside, far])


def inside_points(surface, n, seed=11):
    """Points strictly inside a triangle: min |d| over the three edge functions > 1e-9 x the triangle's area (d and the
    area computed here).  Returns the points and the triangle of each as a sorted vertex triple."""
    rng = np.random.default_rng(seed)
    v = surface.arrays()["vertices"][:, :2]
    tris = triangles(surface)
    pts, owner = [], []
    while len(pts) < n:
        t = tris[rng.integers(len(tris))]
        w = rng.dirichlet([1.0, 1.0, 1.0])
        p = w @ v[list(t)]
        a, b, c = v[list(t)]
        area = 0.5 * abs((b[0] - a[0]) * (c[1] - a[1]) - (c[0] - a[0]) * (b[1] - a[1]))
        d = [(p[0] - q[0]) * (r[1] - q[1]) - (r[0] - q[0]) * (p[1] - q[1]) for q, r in ((a, b), (b, c), (c, a))]
        if min(abs(x) for x in d) > 1e-9 * area and (all(x > 0 for x in d) or all(x < 0 for x in d)):
            pts.append(p)
            owner.append(t)
    return np.array(pts), owner


def vertex_sets(tri):
    return [tuple(sorted(int(x) for x in t)) if t[0] != NONE else None for t in tri]


def counts_by_triangle(rows):
    """Rows folded by the triangle's vertex set (a triangle is named by each of its three edges, so one triangle may hold
    several rows)."""
    out = {}
    for t, c in zip(vertex_sets(rows[0]), rows[1]):
        out[t] = out.get(t, 0) + int(c)
    return out


# ------------------------------------------------------------------------------------------ the DENSE_MESH_RELAX state
def relax_scene(name):
    """(camera positions, ground function, cloud): a camera grid with MODEL_600 over rolling ground and the dense cloud
    sampled from the ground plus noise.  'early' ends because a run creates nothing; 'capped' - rougher ground, cameras
    close to it (a small gsd, so small triangles are allowed) and a patch of 1 m x 1 m where the cloud is very dense - is
    still creating triangles in run 20, so the cap ends it."""
    rows, cols, spacing, height, amp, per_side, noise, seed, patch = SCENES[name]
    rng = np.random.default_rng(seed)
    pos = np.array([[c * spacing + rng.uniform(-0.1, 0.1), r * spacing + rng.uniform(-0.1, 0.1), height]
                    for r in range(rows) for c in range(cols)])
    ground = lambda x, y: 1e-3 * x + 1e-2 * y + amp * np.sin(x / 2.2) * np.cos(y / 2.7)
    gx = np.linspace(-spacing, cols * spacing, per_side)
    gy = np.linspace(-spacing, rows * spacing, per_side)
    X, Y = np.meshgrid(gx, gy, indexing="ij")
    xy = np.stack([X.ravel(), Y.ravel()], -1) + rng.uniform(-0.4, 0.4, (per_side * per_side, 2)) * (gx[1] - gx[0])
    xy = np.concatenate([xy, rng.uniform(0.0, 1.0, (patch, 2)) + [0.37 * cols * spacing, 0.41 * rows * spacing]])
    cloud = np.concatenate([xy, (ground(xy[:, 0], xy[:, 1]) + rng.normal(0, noise, len(xy)))[:, None]], axis=1)
    return pos, ground, cloud


SCENES = {"early": (4, 5, 2.0, 10.0, 0.35, 60, 0.002, 4, 0), "capped": (4, 5, 40.0, 0.9, 0.8, 40, 0.004, 9, 12000)}


def scene_graph(pos):
    ori = np.array([DOWN for _ in pos])
    return host_graph_from_edges(host, pos, ori, MODEL_600, [])


def scene_surface(pos, ground, cloud):
    s = host.rebuild_mesh(pos, minimal=True)
    v = s.arrays()["vertices"]
    s.set_heights(ground(v[:, 0], v[:, 1]))
    s.set_clouds([cloud])
    return s


def oracle_dense_mesh_relax(mesh, clouds, pos, model, max_steps):
    """Pipeline::Impl::dense_mesh_relax (src/pipeline/pipeline.cpp:844-924) written out over the oracle's pieces, sums in
    the reference's order.  pos: the usable cameras' positions (none: gsd 0.01, reduced gsd 0)."""
    log, run = [], 0
    while len(log) < max_steps:
        v, e = mesh.arrays()
        mean_surface_z = 0.0
        for z in v[:, 2]:
            mean_surface_z += float(z)
        if len(v):
            mean_surface_z /= len(v)
        cam_z = arc = size = 0.0
        for p in pos:
            cam_z += float(p[2])
            arc += 1.0 / float(model[0])
            size += float(max(model[8], model[9]))
        gsd, reduced = 0.01, 0.0
        if len(pos):
            cam_z /= len(pos)
            arc /= len(pos)
            size /= len(pos)
            gsd = max(0.001, abs(cam_z - mean_surface_z) * arc)
            reduced = float(np.sqrt(20 / 8.0)) * 0.05 * size * gsd
        stddev = 2.0 * gsd
        min_var = stddev * stddev
        created, above = 0, 0
        if len(v):
            tri, count, var = mesh.count_points_per_triangle(clouds)
            above = int(np.sum((count > 20) & (var > min_var)))
            created = mesh.refine_by_point_density(clouds, 20, min_var, 1, reduced)
        log.append(dict(run=run, gsd=gsd, reduced_gsd=reduced, above_threshold=above, created=created, vertices=len(mesh.arrays()[0])))
        if created > 0 and run < 20:
            run += 1
            continue
        break
    return log


def same_log(log, olog):
    keys = ("run", "gsd", "reduced_gsd", "above_threshold", "created", "vertices")
    return len(log) == len(olog) and all(np.float64(a[k]).view(np.uint64) == np.float64(b[k]).view(np.uint64)
                                         for a, b in zip(log, olog) for k in keys)

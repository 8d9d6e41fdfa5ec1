"""Scenes for the orthomosaic preview and DSM tests (test_ortho_host.py, test_gpu_ortho.py): the reference's own
fixtures of test/test_ortho.cpp restated with their values, and perturbed / refined meshes with a numpy brute-force
height for checking the rasters."""
import numpy as np

from opencalibration_amd import host


def quat(axis, angle):
    """Eigen::Quaterniond(Eigen::AngleAxisd(angle, axis)) as x y z w."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([a * np.sin(angle / 2), [np.cos(angle / 2)]])


def qmul(a, b):
    """Hamilton product of two x y z w quaternions (Eigen's operator*)."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


DOWN = quat((1, 0, 0), np.pi)


def make_graph(positions, orientations, model10, thumbnails=None):
    """A graph of feature-less nodes with the given poses, one camera model and (optionally) a thumbnail per node."""
    g = host.Graph()
    m = g.add_model(np.asarray(model10, np.float64))
    for p in positions:
        g.add_image(np.zeros((0, 2)), np.zeros(0, np.float32), np.zeros((0, 8), np.uint64), 0, m, np.asarray(p, np.float64))
    g.set_orientations(np.asarray(orientations, np.float64).reshape(-1, 4))
    for i, t in enumerate(thumbnails or []):
        if t is not None:
            g.set_thumbnail(i, t)
    return g


def three_cameras():
    """init_cameras of test/test_ortho.cpp:37-82: f 600, principal point (400, 300), 800 x 600, three 100 x 100 thumbnails
    whose layer j of node i holds i * 3 + j."""
    ori = [qmul(quat((0, 0, 1), 0.2), DOWN), qmul(quat((0, 1, 0), -0.3), DOWN), qmul(quat((1, 0, 0), -0.3), DOWN)]
    pos = [(9, 9, 9), (11, 9, 9), (11, 11, 9)]
    model = [600, 400, 300, 0, 0, 0, 0, 0, 800, 600]
    thumbs = [np.broadcast_to(np.array([3 * i, 3 * i + 1, 3 * i + 2], np.uint8), (100, 100, 3)) for i in range(3)]
    return pos, ori, model, thumbs


def cloud_surface(points):
    s = host.Surface()
    s.set_clouds([np.asarray(points, np.float64)])
    return s


def functional_scene():
    """functional_ortho_scene of test/test_ortho.cpp:290-374: two downward cameras at (0, 0, 10) (red) and (10, 0, 10)
    (blue), f 500, 100 x 100, and the mesh rebuilt from them over a flat cloud."""
    model = [500, 50, 50, 0, 0, 0, 0, 0, 100, 100]
    pos = [(0, 0, 10), (10, 0, 10)]
    red = np.zeros((100, 100, 3), np.uint8)
    red[..., 0] = 255
    blue = np.zeros((100, 100, 3), np.uint8)
    blue[..., 2] = 255
    g = make_graph(pos, [DOWN, DOWN], model, [red, blue])
    pts = cloud_surface([(-2, -2, 0), (12, -2, 0), (12, 2, 0), (-2, 2, 0), (5, 0, 0)])
    return g, host.rebuild_mesh(np.array(pos, np.float64), previous=pts)


def jittered_cameras(nx, ny, spacing=10.0, height=40.0, seed=0):
    """A grid of downward cameras with jittered positions (no two kNN distances tie) and small tilts."""
    rng = np.random.default_rng(seed)
    pos = np.array([(x * spacing, y * spacing, height) for y in range(ny) for x in range(nx)], np.float64)
    pos += rng.uniform(-0.3 * spacing, 0.3 * spacing, pos.shape) * np.array([1, 1, 0.05])
    ori = [qmul(quat(rng.normal(size=3), rng.uniform(0, 0.05)), DOWN) for _ in range(len(pos))]
    return pos, np.array(ori)


def perturbed_mesh(pos, seed=1, amplitude=3.0):
    """rebuildMesh over the camera positions with every vertex height perturbed."""
    s = host.rebuild_mesh(pos)
    v = s.arrays()["vertices"]
    rng = np.random.default_rng(seed)
    s.set_heights(v[:, 2] - 40.0 + rng.uniform(-amplitude, amplitude, len(v)))
    return s


def mesh_triangles(surface):
    """The mesh's triangles as (n, 3) vertex indices (ascending, unique) and the vertices."""
    a = surface.arrays()
    v, e = a["vertices"], a["edges"]
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    tris = set()
    for src, dst, _, o0, o1 in e:
        for o in (o0, o1):
            if o != none:
                tris.add(tuple(sorted((int(src), int(dst), int(o)))))
    return np.array(sorted(tris), np.int64), v


def brute_force_heights(surface, xs, ys):
    """Per (x, y) the height of the mesh by barycentric interpolation in any triangle that holds the point (NaN: none)."""
    tris, v = mesh_triangles(surface)
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    det = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (c[:, 0] - a[:, 0]) * (b[:, 1] - a[:, 1])
    z = np.full(xs.shape, np.nan)
    for idx in np.ndindex(xs.shape):
        x, y = xs[idx], ys[idx]
        l1 = ((x - a[:, 0]) * (c[:, 1] - a[:, 1]) - (c[:, 0] - a[:, 0]) * (y - a[:, 1])) / det
        l2 = ((b[:, 0] - a[:, 0]) * (y - a[:, 1]) - (x - a[:, 0]) * (b[:, 1] - a[:, 1])) / det
        l0 = 1 - l1 - l2
        inside = np.nonzero((l0 >= -1e-12) & (l1 >= -1e-12) & (l2 >= -1e-12))[0]
        if len(inside):
            t = inside[0]
            z[idx] = l0[t] * a[t, 2] + l1[t] * b[t, 2] + l2[t] * c[t, 2]
    return z


def pixel_centres(plan, row0=0, rows=None):
    rows = plan["height"] - row0 if rows is None else rows
    r = np.arange(row0, row0 + rows, dtype=np.float64)[:, None]
    c = np.arange(plan["width"], dtype=np.float64)[None, :]
    xs = c * plan["gsd"] + plan["min_x"] + 0 * r
    ys = plan["max_y"] - r * plan["gsd"] + 0 * c
    return xs, ys


def plan_over(surface, gsd, mean_camera_z=60.0, pad=2.0):
    """A raster plan over the surface's bounds (pad beyond them on every side, so that some pixels miss)."""
    b = host.ortho_bounds([surface])
    min_x, max_x, min_y, max_y = b["min_x"] - pad, b["max_x"] + pad, b["min_y"] - pad, b["max_y"] + pad
    return dict(width=int((max_x - min_x) / gsd), height=int((max_y - min_y) / gsd), gsd=gsd, min_x=min_x, max_x=max_x,
                min_y=min_y, max_y=max_y, mean_camera_z=mean_camera_z)


def project(point, position, orientation, model10):
    """image_from_3d(point, model, position, orientation) of the reference (include/opencalibration/distort/
    distort_keypoints.hpp:26-86) in numpy: the point in the camera frame (the conjugate rotation), PLANAR with z clamped
    to 1e-3, distortProjectedRay, * f + principal point."""
    x, y, z, w = np.asarray(orientation, np.float64) / np.linalg.norm(orientation)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    ray = R.T @ (np.asarray(point, np.float64) - np.asarray(position, np.float64))
    f, ppx, ppy, k1, k2, k3, p1, p2 = model10[:8]
    p = ray[:2] / max(ray[2], 1e-3)
    r2 = p @ p
    radial = k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    t = np.array([p1, p2])
    d = (1 + radial) * p + 2 * p[0] * p[1] * t + t[::-1] * (r2 + 2 * p * p)
    return d * f + np.array([ppx, ppy])

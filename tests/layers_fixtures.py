"""Scenes for the layered orthomosaic tests (test_ortho_layers_host.py, test_gpu_ortho_layers.py): small camera sets with
lens distortion over rebuilt meshes, seeded noise images, and a numpy restatement of the per-pixel camera choice."""
import numpy as np

from ortho_fixtures import DOWN, cloud_surface, make_graph, project, qmul, quat
from opencalibration_amd import host

DISTORTED = [100, 80, 60, -0.05, 0.01, 0, 0.001, -0.0005, 160, 120]  # f ppx ppy k1 k2 k3 p1 p2 cols rows


def noise_images(n, rows, cols, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8) for _ in range(n)]


def four_camera_scene(seed=0):
    """Four slightly tilted downward cameras 10 m over a flat mesh, f 100, 160 x 120 with distortion; a noise image each."""
    pos = [(0, 0, 10), (6, 0.3, 10), (0.2, 5, 10.5), (6.5, 5.2, 9.5)]
    rng = np.random.default_rng(seed)
    ori = [qmul(quat(rng.normal(size=3), 0.04), DOWN) for _ in pos]
    g = make_graph(pos, ori, DISTORTED)
    pts = cloud_surface([(-4, -4, 0), (10, -4, 0), (10, 9, 0), (-4, 9, 0), (3, 2.5, 0.5)])
    s = host.rebuild_mesh(np.array(pos, np.float64), previous=pts)
    return g, s, noise_images(len(pos), 120, 160, seed)


def plan_with_gsd(plan, gsd):
    """The plan's bounds at another gsd (the single-pixel path / the radius cap)."""
    p = dict(plan)
    p["gsd"] = gsd
    p["width"] = int((p["max_x"] - p["min_x"]) / gsd)
    p["height"] = int((p["max_y"] - p["min_y"]) / gsd)
    return p


def expected_layers(plan, cams, orientations, positions, models10, dsm, num_layers, row0=0, order_in=None):
    """numpy: per pixel the brute-force 5 nearest cameras (squared XY distance, then index) and the cameras the layers
    take (in front, projected inside the image); returns knn (rows, cols, 5) and layer camera indices (L, rows, cols),
    -1 where invalid.  order_in (rows, cols, 5): walk this camera order instead of numpy's own."""
    rows, cols = dsm.shape
    xs = np.arange(cols) * plan["gsd"] + plan["min_x"]
    ys = plan["max_y"] - np.arange(row0, row0 + rows) * plan["gsd"]
    cxy = cams[:, :2]
    knn = np.full((rows, cols, 5), 0xFFFFFFFF, np.uint32)
    layers = np.full((num_layers, rows, cols), -1, np.int64)
    for r in range(rows):
        d = (xs[:, None] - cxy[None, :, 0]) ** 2 + (ys[r] - cxy[None, :, 1]) ** 2
        order = np.argsort(d, axis=1, kind="stable")[:, :5]
        knn[r, :, :order.shape[1]] = order
        if order_in is not None:
            order = order_in[r].astype(np.int64)
        for c in range(cols):
            z = dsm[r, c]
            if np.isnan(z):
                continue
            p = np.array([xs[c], ys[r], float(z)])
            k = 0
            for i in order[c]:
                if i < 0 or i >= len(cams):
                    break
                if k >= num_layers:
                    break
                R = cams[i, 3:12].reshape(3, 3)
                if (R @ (p - positions[i]))[2] <= 0:
                    continue
                px = project(p, positions[i], orientations[i], models10[i])
                w, h = models10[i][8], models10[i][9]
                if not (0 <= px[0] < w and 0 <= px[1] < h):
                    continue
                layers[k, r, c] = i
                k += 1
    return knn, layers


def knn_agrees(got, expected, plan, cams, row0=0):
    """the kNN lists are equal except where two cameras swap places at a distance tie within 1e-12 (numpy's and C's
    squared distances may round apart there)"""
    bad = np.nonzero((got != expected).any(-1))
    for r, c in zip(*bad):
        x, y = c * plan["gsd"] + plan["min_x"], plan["max_y"] - (row0 + r) * plan["gsd"]
        d = lambda i: (x - cams[i, 0]) ** 2 + (y - cams[i, 1]) ** 2
        if sorted(got[r, c].tolist()) != sorted(expected[r, c].tolist()):
            return False
        for a, b in zip(got[r, c], expected[r, c]):
            if a != b and abs(d(a) - d(b)) > 1e-12 * d(a):
                return False
    return len(bad[0]) <= 0.001 * got.shape[0] * got.shape[1] + 2

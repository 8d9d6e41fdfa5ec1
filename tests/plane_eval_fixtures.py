"""Seeded problems of the plane relax engine (ochip_relax_desc, as dicts of its fields: capi.relax_desc) for the evaluation
tests, and their restatement as general-engine scenes (to_relaxg) for the long-double oracle (oracle/relax_eval.cpp).  The
bounds are those of tests/relax_eval_fixtures.py (c = 2^18), the cost compared as the reduced program's.  Data and
arithmetic only; no device.

Mapping of a plane problem onto a relaxg scene: vertices 0-2 are the corners (plane_xy, plane_z, z_optimize), one triangle
(0, 1, 2), every block a 2-ray block on it with ray_cam = (a, b), down_cam = prior_cam, down_weight = prior_weight, the same
huber_a, no other prior; cameras constant is structure_only."""
import numpy as np

import relax_eval_fixtures as G
from relax_fixtures import DOWN, axis_angle, qinv, qmul, qrot

HUBER_A = G.HUBER_A


def to_plane(s):
    """the ochip_relax_desc fields of a relaxg scene of the plane shape (relax_eval_fixtures.plane)"""
    assert np.all(np.asarray(s["blk_n"]) == 2) and np.all(np.asarray(s["blk_tri"]).reshape(-1, 3) == [0, 1, 2])
    rc = np.asarray(s["ray_cam"], np.uint32).reshape(-1, 2)
    return dict(cam_pos=np.asarray(s["cam_pos"], float), cam_q=np.asarray(s["cam_q"], float),
                cam_optimize=np.asarray(s["cam_optimize"], np.uint8), plane_xy=np.asarray(s["vert_xy"], float)[:3].reshape(-1),
                plane_z=np.asarray(s["vert_z"], float)[:3], z_optimize=np.asarray(s["vert_optimize"], np.uint8)[:3],
                blk_cam_a=rc[:, 0].copy(), blk_cam_b=rc[:, 1].copy(), blk_rays=np.asarray(s["ray_dir"], float).reshape(-1, 6),
                prior_cam=np.asarray(s["down_cam"], np.uint32), huber_a=float(s["huber_a"]), prior_weight=float(s["down_weight"]))


def to_relaxg(p, cam_q=None, plane_z=None):
    """the relaxg scene of a plane problem (mapping: head of this file), at the state (cam_q, plane_z) when given"""
    nb = len(p["blk_cam_a"])
    return dict(cam_pos=p["cam_pos"], cam_q=p["cam_q"] if cam_q is None else cam_q, cam_optimize=p["cam_optimize"],
                vert_xy=np.asarray(p["plane_xy"], float).reshape(3, 2),
                vert_z=np.asarray(p["plane_z"] if plane_z is None else plane_z, float),
                vert_optimize=np.asarray(p["z_optimize"], np.uint8), blk_n=np.full(nb, 2, np.uint8),
                blk_intr=np.zeros(nb, np.uint8), blk_ray_off=(2 * np.arange(nb + 1)).astype(np.uint32),
                blk_tri=np.tile(np.arange(3, dtype=np.uint32), nb),
                ray_cam=np.stack([p["blk_cam_a"], p["blk_cam_b"]], 1).astype(np.uint32).reshape(-1),
                ray_dir=np.asarray(p["blk_rays"], float).reshape(-1), ray_px=None, down_cam=np.asarray(p["prior_cam"], np.uint32),
                down_weight=p["prior_weight"], diff_v=np.zeros(0, np.uint32), diff_weight=0.0, anchor_weight=0.0,
                huber_a=p["huber_a"], model=G.MODEL)


class Builder:
    """cameras at height 10 looking down (perturbed by 0.03 rad) at the given xy, a plane through three corners; a block
    is the two cameras' rays to a ground point between them"""

    def __init__(self, seed, cam_xy, spacing=4.0):
        self.rng = rng = np.random.default_rng(seed)
        cam_xy = np.asarray(cam_xy, float)
        n = len(cam_xy)
        self.cam = np.concatenate([cam_xy, np.full((n, 1), 10.0)], 1)
        self.q = np.array([qmul(DOWN, axis_angle(a / np.linalg.norm(a), 0.03)) for a in rng.normal(size=(n, 3))])
        lo, hi = cam_xy.min(0) - spacing, cam_xy.max(0) + spacing
        hi = lo + 2 * (hi - lo)  # (a triangle that holds the cameras' square: the ground points interpolate the corners)
        self.xy = np.array([[lo[0], lo[1]], [hi[0], lo[1]], [lo[0], hi[1]]])
        self.z = rng.normal(size=3) * 0.3
        self.spacing = spacing
        self.a, self.b, self.rays = [], [], []

    def z_at(self, xy):
        (x0, y0), (x1, _), (_, y2) = self.xy
        u, v = (xy[0] - x0) / (x1 - x0), (xy[1] - y0) / (y2 - y0)
        return self.z[0] + u * (self.z[1] - self.z[0]) + v * (self.z[2] - self.z[0])

    def block(self, a, b, noise):
        rng = self.rng
        xy = (self.cam[a, :2] + self.cam[b, :2]) / 2 + rng.normal(size=2) * 0.3 * self.spacing
        p = np.array([*xy, self.z_at(xy) + rng.normal() * 0.05])
        rays = []
        for c in (a, b):
            d = qrot(qinv(self.q[c]), (p - self.cam[c]) / np.linalg.norm(p - self.cam[c]))
            rays.append(G._rot_noise(rng, d, noise))
        self.a.append(a)
        self.b.append(b)
        self.rays.append(np.concatenate(rays))

    def link(self, a, b, k, noise=(1e-3, 3e-2)):
        for i in range(k):
            self.block(a, b, noise[i % len(noise)])

    def desc(self, cam_optimize=None, z_optimize=(1, 1, 1), prior_cam=None, huber_a=HUBER_A):
        n = len(self.cam)
        return dict(cam_pos=self.cam, cam_q=self.q,
                    cam_optimize=np.ones(n, np.uint8) if cam_optimize is None else np.asarray(cam_optimize, np.uint8),
                    plane_xy=self.xy.reshape(-1), plane_z=self.z.copy(), z_optimize=np.asarray(z_optimize, np.uint8),
                    blk_cam_a=np.array(self.a, np.uint32), blk_cam_b=np.array(self.b, np.uint32),
                    blk_rays=np.array(self.rays).reshape(-1, 6), huber_a=huber_a, prior_weight=1e-3,
                    prior_cam=np.arange(n, dtype=np.uint32) if prior_cam is None else np.asarray(prior_cam, np.uint32))


def grid(rows, cols, seed, per_link=2, shuffle=False, **kw):
    """rows x cols cameras linked to their right and lower neighbours by per_link blocks each; shuffle: the camera
    indices in a random order (the engine renumbers them)"""
    rng = np.random.default_rng(seed + 1000)
    perm = rng.permutation(rows * cols) if shuffle else np.arange(rows * cols)
    xy = np.zeros((rows * cols, 2))
    for r in range(rows):
        for c in range(cols):
            xy[perm[r * cols + c]] = (4.0 * (c - cols // 2), 4.0 * (r - rows // 2))
    B = Builder(seed, xy)
    for r in range(rows):
        for c in range(cols):
            i = perm[r * cols + c]
            if c + 1 < cols:
                B.link(i, perm[r * cols + c + 1], per_link)
            if r + 1 < rows:
                B.link(perm[(r + 1) * cols + c], i, per_link)  # (listed as (b, a) as often as (a, b))
    return B.desc(**kw)


def plane():
    """relax_eval_fixtures.plane(): pairs of 1, 63, 64, 65 and 200 blocks, one listed as (b, a), a constant camera with a
    prior, a camera with a prior only, the middle corner constant"""
    return to_plane(G.plane())


def plane_iterated():
    """plane() without the prior of camera 6 (its only block): the iterated cases carry no camera held by its prior alone.
    The solve turns such a camera straight down, where PointsDownwardsPrior's acos of a dot product near 1 loses its
    digits in fp64 (tests/test_plane_eval_oracle.py, test_downward_prior_near_straight_down)."""
    p = plane()
    p["prior_cam"] = p["prior_cam"][p["prior_cam"] != 6]
    return p


def huber_edge(side, seed=6):
    """block 0's s at a^2 (1 + 1e-5) (side > 0: the linear branch) or a^2 (1 - 1e-5)"""
    from oracle import pyoracle

    B = Builder(seed, [(0, 0), (4, 0), (0, 4)])
    for i in range(6):
        B.block(i % 3, (i + 1) % 3, 2e-2)
    p = B.desc()
    e = pyoracle.relaxg_eval(to_relaxg(p), raw=True)
    r0 = e["r"][e["row_blk"] == 0]
    p["huber_a"] = float(np.sqrt(np.dot(r0, r0) / (1 + 1e-5 * side)))
    return p


def priors_only(seed=8):
    """no blocks at all: the priors alone, so there are no height unknowns"""
    return Builder(seed, [(0, 0), (4, 0), (0, 4), (4, 4)]).desc()


def fixed_pair(seed=9):
    """every height constant and a pair of two constant cameras (4, 5): blocks that read no unknown"""
    B = Builder(seed, [(4.0 * i, 0.0) for i in range(6)])
    for a, k in zip(range(5), (5, 7, 3, 6, 9)):
        B.link(a, a + 1, k)
    return B.desc(cam_optimize=[1, 1, 1, 1, 0, 0], z_optimize=(0, 0, 0))


def n64(seed=10):
    """21 cameras in a 7 x 3 grid and one free height: n = 64"""
    return grid(3, 7, seed, z_optimize=(0, 1, 0))


def renumbered(seed=11):
    """63 cameras (more than 42) in shuffled order, three free heights: the renumbering, n = 192"""
    return grid(7, 9, seed, shuffle=True)


def dissected(seed=17):
    """256 cameras in a 16 x 16 grid, shuffled, 2 blocks per link (960 blocks): the camera graph cut into regions and
    separators, n = 771"""
    return grid(16, 16, seed, shuffle=True)


def failing(seed=13):
    """a ray parallel to the plane: the intersection fails"""
    B = Builder(seed, [(0, 0), (4, 0), (0, 4)])
    B.z[:] = 0
    for i in range(4):
        B.block(i % 3, (i + 1) % 3, 1e-3)
    B.rays[3][3:] = qrot(qinv(B.q[B.b[3]]), np.array([1.0, 0.0, 0.0]))
    return B.desc()


def cases():
    """(name, plane problem)"""
    return [("plane", plane()), ("huber_above", huber_edge(+1)), ("huber_below", huber_edge(-1)),
            ("priors_only", priors_only()), ("fixed_pair", fixed_pair()), ("n64", n64()), ("renumbered", renumbered())]


def big_cases():
    return [("dissected", dissected())]


def reduced(ref):
    """a long-double evaluation with its cost replaced by the reduced program's (what the plane engine reports)"""
    return dict(ref, cost=ref["cost_reduced"])


def huber_margin(p, delta=None, structure_only=False, cam_q=None, plane_z=None):
    """smallest | s / a^2 - 1 | over the blocks (raw long-double residuals), inf without blocks"""
    from oracle import pyoracle

    if len(p["blk_cam_a"]) == 0:
        return np.inf
    e = pyoracle.relaxg_eval(to_relaxg(p, cam_q, plane_z), raw=True, delta=delta, structure_only=structure_only)
    sq = np.bincount(e["row_blk"], weights=e["r"] ** 2)[:len(p["blk_cam_a"])]
    return float(np.min(np.abs(sq / p["huber_a"] ** 2 - 1)))

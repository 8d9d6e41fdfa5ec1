"""Small seeded problems of the general relax engine (ochip_relaxg_desc, as dicts of its fields: capi.relaxg_desc) for the
evaluation tests, and the normwise bounds the device's and the fp64 oracle's J'J, J'r and cost are held to against the
long-double oracle (oracle/relax_eval.cpp).  Data and arithmetic only; no device."""
import numpy as np

from relax_fixtures import DOWN, axis_angle, qinv, qmul, qrot

U = 2.0 ** -53
C_BOUND = 2.0 ** 18  # the one constant of every bound (calibration: tests/test_relax_eval_oracle.py)
HUBER_A = np.deg2rad(1.0)
MODEL = np.array([1000.0, 500.0, 400.0, -0.02, 0.01, -0.005, 1e-4, -2e-4])


def _rot_noise(rng, v, ang):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    return qrot(axis_angle(ax, ang), v)


class Builder:
    """cameras on a grid at height 10 looking down (perturbed), a mesh x mesh ground mesh, ray blocks added one by one"""

    def __init__(self, seed, n_cams=5, mesh=3, spacing=4.0, model=MODEL):
        self.rng = rng = np.random.default_rng(seed)
        cols = int(np.ceil(np.sqrt(n_cams)))
        self.cam = np.array([[(i % cols) * spacing, (i // cols) * spacing, 10.0] for i in range(n_cams)])
        self.q = np.array([qmul(DOWN, axis_angle(a / np.linalg.norm(a), 0.03)) for a in rng.normal(size=(n_cams, 3))])
        ext = max(cols, (n_cams + cols - 1) // cols) * spacing
        vx, vy = np.meshgrid(np.linspace(-spacing, ext, mesh), np.linspace(-spacing, ext, mesh))
        self.vxy = np.stack([vx.ravel(), vy.ravel()], 1)
        self.vz = rng.normal(size=mesh * mesh) * 0.3
        self.mesh = mesh
        tris = []
        for r in range(mesh - 1):
            for c in range(mesh - 1):
                a, b, d, e = mesh * r + c, mesh * r + c + 1, mesh * (r + 1) + c, mesh * (r + 1) + c + 1
                tris += [(a, b, e), (a, e, d)]
        self.tris = np.array(tris)
        self.model = np.array(model, float)
        self.blk_n, self.blk_intr, self.blk_tri, self.ray_cam, self.ray_dir, self.ray_px = [], [], [], [], [], []
        self.extra = {}

    def block(self, cams, intr=False, noise=1e-3, outlier=None, tri=None):
        """a block of the rays of `cams` through one ground point; every ray turned by `noise` rad, ray `outlier` by 0.05"""
        rng = self.rng
        k = int(rng.integers(len(self.tris))) if tri is None else tri
        t = self.tris[k]
        w = rng.dirichlet([4, 4, 4])
        p = np.array([*(w @ self.vxy[t]), w @ self.vz[t] + rng.normal() * 0.05])
        self.blk_n.append(len(cams))
        self.blk_intr.append(int(intr))
        self.blk_tri.append(t)
        for i, c in enumerate(cams):
            d = qrot(qinv(self.q[c]), (p - self.cam[c]) / np.linalg.norm(p - self.cam[c]))
            d = _rot_noise(rng, d, 0.05 if i == outlier else noise)
            self.ray_cam.append(c)
            self.ray_dir.append(d)
            self.ray_px.append(d[:2] / d[2] * self.model[0] + self.model[1:3])
        return len(self.blk_n) - 1

    def scene(self, down=True, diff=True, anchor=True, smooth=False, mono=0, rel=0, opt=(0, 0, 0), cam_optimize=None,
              vert_optimize=None, huber_a=HUBER_A):
        n_cams, m = len(self.cam), self.mesh
        diff_v = [(m * r + c, m * r + c + 1) for r in range(m) for c in range(m - 1)] + \
                 [(m * r + c, m * (r + 1) + c) for r in range(m - 1) for c in range(m)]
        used = sorted(set(self.ray_cam)) if self.ray_cam else list(range(n_cams))
        s = dict(cam_pos=self.cam, cam_q=self.q, vert_xy=self.vxy, vert_z=self.vz,
                 cam_optimize=np.ones(n_cams, np.uint8) if cam_optimize is None else np.asarray(cam_optimize, np.uint8),
                 vert_optimize=np.ones(len(self.vz), np.uint8) if vert_optimize is None else np.asarray(vert_optimize, np.uint8),
                 blk_n=np.array(self.blk_n, np.uint8), blk_intr=np.array(self.blk_intr, np.uint8),
                 blk_ray_off=np.concatenate([[0], np.cumsum(self.blk_n)]).astype(np.uint32),
                 blk_tri=np.array(self.blk_tri, np.uint32).reshape(-1), ray_cam=np.array(self.ray_cam, np.uint32),
                 ray_dir=np.array(self.ray_dir).reshape(-1), ray_px=np.array(self.ray_px).reshape(-1),
                 down_cam=np.array(used if down else [], np.uint32), down_weight=1e-3,
                 diff_v=np.array(diff_v if diff else [], np.uint32).reshape(-1), diff_weight=1e-4,
                 anchor_weight=1e-5 if anchor else 0.0, huber_a=huber_a, model=self.model,
                 opt_focal=opt[0], opt_principal=opt[1], n_radial_free=opt[2])
        if smooth:  # every inner mesh edge of the two triangles of a grid cell: A B (the diagonal), C D
            sv = []
            for r in range(m - 1):
                for c in range(m - 1):
                    a, b, d, e = m * r + c, m * r + c + 1, m * (r + 1) + c, m * (r + 1) + c + 1
                    sv.append((a, e, b, d))
            s.update(smooth_v=np.array(sv, np.uint32).reshape(-1), smooth_weight=1e-4)
        if mono:
            s.update(mono_observations=mono, mono_r_max=3.0)
        if rel:
            rng = self.rng
            rc, poses = [], []
            for i in range(rel):
                a, b = (i % n_cams), (i + 1) % n_cams
                rc.append((a, b))
                blk = []
                for k, score in enumerate((50, 40, 5, 0)):
                    ax = rng.normal(size=3)
                    qr = axis_angle(ax / np.linalg.norm(ax), 0.3 + 0.2 * k)
                    t = rng.normal(size=3)
                    blk.append([*qr, *(t / np.linalg.norm(t)), score])
                poses.append(blk)
            s.update(rel_cam=np.array(rc, np.uint32).reshape(-1), rel_pose=np.array(poses).reshape(-1),
                     rel_huber_a=np.deg2rad(10.0))
        s.update(self.extra)
        return s


def mixed(seed=1, opt=(1, 1, 2), intr=True):
    """every record type on a banded 3 x 3 mesh: 2..5-ray blocks with and without intrinsics, some with one outlier ray (the
    robust centroid reweights), 2-ray blocks on both sides of the Huber threshold, every prior, a constant camera, a camera
    without blocks (its prior only), a constant vertex"""
    B = Builder(seed, n_cams=7, mesh=3)
    for i in range(24):
        a, b = int(B.rng.integers(6)), int(B.rng.integers(6))
        b = (a + 1 + b % 5) % 6
        B.block([a, b] if i % 2 else [b, a], intr=intr and i % 3 == 0, noise=[3e-4, 1e-2, 4e-2][i % 3])
    for N in (3, 4, 5):
        for j in range(6):
            cams = list(B.rng.choice(6, N, replace=False))
            B.block(cams, intr=intr and j % 2 == 1, noise=2e-3, outlier=(0 if j < 4 else None))
    vo = np.ones(9, np.uint8)
    vo[4] = 0
    co = np.ones(7, np.uint8)
    co[5] = 0
    s = B.scene(smooth=True, mono=40 if opt[2] else 0, rel=3, opt=opt, cam_optimize=co, vert_optimize=vo)
    s["down_cam"] = np.array([0, 1, 2, 3, 4, 5, 6], np.uint32)  # camera 6 has no ray block: the prior alone
    return s


def tail_intr(opt, seed=2):
    """a 2 x 2 mesh (the dense tail) and intrinsics blocks of 2..5 rays under one (opt_focal, opt_principal, n_radial_free)"""
    B = Builder(seed, n_cams=5, mesh=2)
    for N in (2, 3, 4, 5):
        for j in range(4):
            B.block(list(B.rng.choice(5, N, replace=False)), intr=j != 3, noise=[1e-3, 3e-2, 5e-3, 1e-3][j])
    return B.scene(mono=25 if opt[2] else 0, opt=opt)


def plane(counts=(1, 63, 64, 65, 200), seed=3):
    """the plane engine's shape: three corner heights (one constant), 2-ray blocks per pair with the given counts (one pair
    listed as (b, a), b > a), a constant camera, a camera without pairs, downward priors"""
    B = Builder(seed, n_cams=7, mesh=2)
    B.vxy, B.vz, B.tris = B.vxy[:3], B.vz[:3], np.array([[0, 1, 2]])
    pairs = [(0, 1), (2, 1), (1, 3), (3, 4), (4, 5)]
    for (a, b), k in zip(pairs, counts):
        for i in range(k):
            B.block([a, b], tri=0, noise=[1e-3, 3e-2][i % 2])
    s = B.scene(diff=False, anchor=False, cam_optimize=[1, 1, 1, 1, 0, 1, 1], vert_optimize=[1, 0, 1])
    s["down_cam"] = np.arange(7, dtype=np.uint32)
    return s


def priors_only(seed=4):
    B = Builder(seed, n_cams=4, mesh=3)
    s = B.scene(smooth=True, mono=30, rel=3, opt=(1, 1, 3))
    s["down_cam"] = np.arange(4, dtype=np.uint32)
    return s


def chunked(band_vertex=False, seed=5):
    """owners with more than 1 024 records: two cameras (band owners, cut into BAND_CHUNK chunks), the mesh heights and the
    intrinsics (tail owners whose records run over many TAIL_CHUNK-capped chunks, the last one partial); band_vertex: a
    3 x 3 mesh whose heights are band owners, all blocks on one triangle"""
    B = Builder(seed, n_cams=3, mesh=3 if band_vertex else 2)
    tri = 0 if band_vertex else None
    for i in range(1100):
        B.block([0, 1], intr=i % 2 == 0, noise=[1e-3, 3e-2][i % 2], tri=tri)
    for i in range(37):
        B.block([1, 2, 0], intr=i % 2 == 1, noise=2e-3, tri=tri)
    return B.scene(anchor=True, opt=(1, 1, 1))


def huber_edge(side, seed=6):
    """one 2-ray block's s at a^2 (1 + 1e-5) (side > 0: the linear branch) or a^2 (1 - 1e-5) (side < 0)"""
    from oracle import pyoracle

    B = Builder(seed, n_cams=3, mesh=2)
    for i in range(6):
        B.block([i % 3, (i + 1) % 3], noise=2e-2)
    s = B.scene()
    e = pyoracle.relaxg_eval(s, raw=True)
    r0 = e["r"][e["row_blk"] == 0]
    s["huber_a"] = float(np.sqrt(np.dot(r0, r0) / (1 + 1e-5 * side)))
    return s


def failing(seed=7):
    """a 2-ray block with one ray parallel to the ground plane: the intersection fails"""
    B = Builder(seed, n_cams=3, mesh=2)
    B.vz[:] = 0
    for i in range(4):
        B.block([0, 1])
    B.ray_dir[3] = qrot(qinv(B.q[1]), np.array([1.0, 0.0, 0.0]))
    return B.scene()


def cases():
    """(name, scene, structure_only)"""
    out = [("mixed", mixed(), False), ("mixed_fixed_intr", mixed(seed=11, intr=False, opt=(0, 0, 0)), False),
           ("mixed_structure_only", mixed(seed=12), True), ("plane", plane(), False), ("priors_only", priors_only(), False),
           ("huber_above", huber_edge(+1), False), ("huber_below", huber_edge(-1), False)]
    for f in (0, 1):
        for p in (0, 1):
            for k in range(4):
                out.append((f"tail_f{f}_pp{p}_k{k}", tail_intr((f, p, k), seed=20 + 8 * f + 4 * p + k), False))
    return out


def big_cases():
    return [("chunked_tail", chunked(), False), ("chunked_band_vertex", chunked(band_vertex=True), False)]


# ---- bounds ------------------------------------------------------------------------------------------------------------
def block_stats(ref):
    """per block of a long-double evaluation: rows, ||J_b||_max (corrected, tangent), ||r_b||_2, the columns it touches"""
    nb = int(ref["row_blk"].max()) + 1 if len(ref["row_blk"]) else 0
    rows = np.bincount(ref["row_blk"], minlength=nb)
    jmax = np.zeros(nb)
    np.maximum.at(jmax, ref["row_blk"], np.abs(ref["J"]).max(axis=1) if ref["n"] else 0)
    rn = np.sqrt(np.bincount(ref["row_blk"], weights=ref["r"] ** 2, minlength=nb))
    touch = np.zeros((nb, ref["n"]))
    np.maximum.at(touch, ref["row_blk"], ref["touch"].astype(float))
    return rows, jmax, rn, touch


def bounds(ref, c=C_BOUND):
    """c u-scaled normwise bounds: J'J_ij: sum_b rows_b ||J_b||^2_max over blocks touching i and j; J'r_i: sum_b
    ||J_b||_max ||r_b|| over blocks touching i; cost: relative to sum_b |cost_b| (= the cost: every term >= 0); J_b:
    ||J_b||_max elementwise.  The elementwise J bound has a heavy tail over blocks: an angle residual of a few 1e-6 rad
    can put one fp64 partial past it (tests/test_plane_eval_oracle.py: four of the first seeds of a 960-block grid did),
    so a larger fixture may need its seed chosen again; the normwise J'J and J'r bounds stay far inside at the same
    states.  J'r's bound scales with ||r_b||: a block fitted to a few 1e-6 rad leaves it to rounding (same file)."""
    rows, jmax, rn, T = block_stats(ref)
    return dict(JtJ=c * U * (T.T @ (T * (rows * jmax ** 2)[:, None])), Jtr=c * U * (T.T @ (jmax * rn)),
                cost=c * U * abs(ref["cost"]), J=c * U * jmax[ref["row_blk"]][:, None] * np.ones((1, ref["n"])))


def ratio(err, bound):
    """largest |err| / bound; an error where the bound is 0 is infinite"""
    err, bound = np.abs(np.asarray(err, float)), np.asarray(bound, float)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
    return float(np.max(r))


def ratios(got, ref, b=None):
    """the worst error-to-bound ratio of cost, J'J and J'r of an evaluation (canonical order) against the reference"""
    b = bounds(ref) if b is None else b
    return dict(cost=ratio(got["cost"] - ref["cost"], b["cost"]), JtJ=ratio(got["JtJ"] - ref["JtJ"], b["JtJ"]),
                Jtr=ratio(got["Jtr"] - ref["Jtr"], b["Jtr"]))

"""Seeded scenes of the resident bootstrap chain (ochip_plane_chain_*, csrc/relax_chain.hip) for the trace tests, the numpy
restatement of a step's set-up (grid filter, block lists, priors, tangent offsets), the reduction of a traced evaluation to
a plane problem (plane_eval_fixtures.to_relaxg then takes it to the long-double oracle), the linear solve's references
(lm_fixtures' bounds on the chain's dense system, a transcription of the one-thread Cholesky of systems up to 12 unknowns)
and a transcription of lm_trust and the termination rules of relax_lm_rules.hpp.  Data and arithmetic only; no device.

A scene: cameras at height 10 looking down, perturbed by about 0.03 rad; ground points on a tilted plane; every match is
the long-double forward projection (radial + tangential: relax_eval_fixtures.MODEL, so image_to_3d's TinySolver runs) of
one ground point into the two cameras of its edge, moved by 1 or 30 pixels (residuals on both sides of the Huber
threshold); a plane-induced H per edge; pairwise distinct descriptor scores.  Every match of an edge lies in a cell of the
source image's grid of its own, so the grid filter keeps all of them and the block count of an edge is its match count."""
import functools

import numpy as np

import lm_fixtures as LM
import relax_eval_fixtures as G

LD = np.longdouble
U = 2.0 ** -53
MODEL10 = np.concatenate([G.MODEL, [1000.0, 800.0]])
GRID = 1.0 / 14.0  # finer than 0.15: 14 x 14 cells per image, up to 392 blocks per edge
CELLS = 14
HUBER_A = G.HUBER_A
TRI = np.array([-15.0, -15.0, 45.0, -15.0, -15.0, 45.0])  # anticlockwise, holds every ground point
Z0 = 0.0
N_SMALL = 12
C_QUAT = 32.0  # the candidate's components against long double: 32 u each (tests/test_lm_rules_host.py)


# ---- quaternions (x, y, z, w), any float type ---------------------------------------------------------------------------
def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def qconj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def qrot(q, v):
    return qmul(qmul(q, np.array([v[0], v[1], v[2], v[0] * 0])), qconj(q))[:3]


def axis_angle(axis, ang):
    axis = np.asarray(axis, float)
    return np.array([*(axis / np.linalg.norm(axis) * np.sin(ang / 2)), np.cos(ang / 2)])


DOWN = axis_angle([1, 0, 0], np.pi)


def project_ld(q, pos, P, model=G.MODEL):
    """pixel of the world point P in the camera (q, pos): distortProjectedRay in long double"""
    ql = np.asarray(q, LD)
    d = qrot(qconj(ql), np.asarray(P, LD) - np.asarray(pos, LD))
    x, y = d[0] / d[2], d[1] / d[2]
    k, tg = np.asarray(model[3:6], LD), np.asarray(model[6:8], LD)
    r2 = x * x + y * y
    radial = k[0] * r2 + k[1] * r2 * r2 + k[2] * r2 * r2 * r2
    rp = (x, y)
    out = [(1 + radial) * rp[i] + 2 * x * y * tg[i] + tg[1 - i] * (r2 + 2 * rp[i] * rp[i]) for i in range(2)]
    return np.array([float(LD(model[0]) * out[0] + LD(model[1])), float(LD(model[0]) * out[1] + LD(model[2]))])


# ---- scenes --------------------------------------------------------------------------------------------------------------
class Scene:
    def __init__(self, name, seed, cam_xy, slope=(0.02, -0.015, 0.2), prior_weight=1e-4, noise=(1.0, 30.0)):
        self.name, self.prior_weight, self.noise = name, prior_weight, noise
        self.rng = rng = np.random.default_rng(seed)
        cam_xy = np.asarray(cam_xy, float)
        n = len(cam_xy)
        self.cam_pos = np.concatenate([cam_xy, np.full((n, 1), 10.0)], 1)
        self.q_true = np.array([qmul(DOWN, axis_angle(a, 0.03)) for a in rng.normal(size=(n, 3))])
        # where the chain starts from: another 0.02 rad away, so that the solves have steps to take
        self.cam_q = np.array([qmul(q, axis_angle(a, 0.02)) for q, a in zip(self.q_true, rng.normal(size=(n, 3)))])
        self.cam_optimize = np.ones(n, np.uint8)
        self.slope = slope
        self.edges, self.inliers, self.steps = [], [], []
        self._scores = iter(rng.permutation(4000) / 8000.0 + 0.25)  # pairwise distinct, in [0.25, 0.75)

    def plane_z(self, x, y):
        return self.slope[2] + self.slope[0] * x + self.slope[1] * y

    def _H(self, a, b):
        """the homography of the true plane from a's normalised coordinates to b's"""
        pts = []
        for u, v in ((-0.2, -0.2), (0.2, -0.2), (0.2, 0.2), (-0.2, 0.2)):
            P = self._ground(a, np.array([u, v, 1.0]))
            d = qrot(qconj(self.q_true[b]), P - self.cam_pos[b])
            pts.append(((u, v), (d[0] / d[2], d[1] / d[2])))
        M = []
        for (x, y), (X, Y) in pts:
            M.append([x, y, 1, 0, 0, 0, -X * x, -X * y, -X])
            M.append([0, 0, 0, x, y, 1, -Y * x, -Y * y, -Y])
        h = np.linalg.svd(np.array(M))[2][-1]
        return h / h[8]

    def _ground(self, a, ray_cam):
        d = qrot(self.q_true[a], ray_cam)
        o = self.cam_pos[a]
        nrm = np.array([-self.slope[0], -self.slope[1], 1.0])
        t = (self.slope[2] - np.dot(nrm, o)) / np.dot(nrm, d)
        return o + t * d

    def edge(self, a, b, k, dead=False, homography=True):
        """k matches of cameras a -> b, each in a cell of a's grid of its own (cells in a seeded order; a cell whose ground
        point b does not see well inside its image is passed over).  dead: descriptor scores below zero - no match scores
        above 0, none is kept, the edge has no block."""
        rng = self.rng
        cw, ch = MODEL10[8] / CELLS, MODEL10[9] / CELLS
        first = len(self.inliers)
        for c in rng.permutation(CELLS * CELLS):
            if len(self.inliers) - first == k:
                break
            cx, cy = c // CELLS, c % CELLS
            u = (cx + 0.5) * cw + rng.uniform(-0.2, 0.2) * cw
            v = (cy + 0.5) * ch + rng.uniform(-0.2, 0.2) * ch
            P = self._ground(a, np.array([(u - MODEL10[1]) / MODEL10[0], (v - MODEL10[2]) / MODEL10[0], 1.0]))
            p1, p2 = project_ld(self.q_true[a], self.cam_pos[a], P), project_ld(self.q_true[b], self.cam_pos[b], P)
            noise = self.noise[(len(self.inliers) - first) % len(self.noise)]
            ang = rng.uniform(0, 2 * np.pi)
            p2 = p2 + noise * np.array([np.cos(ang), np.sin(ang)])
            if not (5 < p2[0] < MODEL10[8] - 5 and 5 < p2[1] < MODEL10[9] - 5):
                continue
            assert int(p1[0] / cw) == cx and int(p1[1] / ch) == cy
            s = next(self._scores)
            self.inliers.append((p1, p2, -s if dead else s))
        assert len(self.inliers) - first == k, (self.name, a, b, k, len(self.inliers) - first)
        self.edges.append(dict(cam_a=a, cam_b=b, n=k, first=first, flags=int(homography), H=self._H(a, b)))
        return len(self.edges) - 1

    def step(self, cam, mode, n_filter, prev_cam=-1, prev_q=None):
        self.steps.append(dict(cam=cam, mode=mode, n_filter=n_filter, prev_cam=prev_cam,
                               prev_q=np.zeros(4) if prev_q is None else np.asarray(prev_q, float)))

    # the arrays ochip_plane_chain_create takes
    def arrays(self):
        from opencalibration_amd import capi

        e = np.zeros(len(self.edges), capi.PLANE_EDGE_DTYPE)
        for i, d in enumerate(self.edges):
            e[i] = (d["cam_a"], d["cam_b"], 0, 0, d["n"], d["flags"], d["first"], d["H"])
        m = np.zeros(len(self.inliers), capi.PLANE_INLIER_DTYPE)
        for i, (p1, p2, s) in enumerate(self.inliers):
            m[i] = (p1, p2, s)
        st = np.zeros(len(self.steps), capi.PLANE_CHAIN_STEP_DTYPE)
        for i, d in enumerate(self.steps):
            st[i] = (d["cam"], d["mode"], d["n_filter"], d["prev_cam"], d["prev_q"], TRI, Z0)
        return dict(edges=e, inliers=m, steps=st, cam_pos=self.cam_pos, cam_q=self.cam_q, cam_optimize=self.cam_optimize,
                    models10=MODEL10[None], grid_fraction=GRID, huber_a=HUBER_A, prior_weight=self.prior_weight)


def _cluster(n, spacing=1.0):
    cols = int(np.ceil(np.sqrt(n)))
    return [((i % cols) * spacing, (i // cols) * spacing) for i in range(n)]


def bootstrap(seed=31):
    """Four steps whose state buffers and system sets alternate: a step without edges (n_filter 0: mode 0, the prior of the
    new camera alone, n = 3 and no heights - the whole step in one epilogue through eval_serial), a mode-0 step against
    oriented neighbours (n = 6), a mode-1 step with prev_cam >= 0 and a mode-2 step (n = 12: cameras 1, 2 and 3; cameras 0
    and 4 constant on shared edges).  Edges of 1, 63, 64, 65 and 130 blocks (three chunks), both orders of the pair (0, 1),
    cam_a > cam_b, an edge without a surviving block (a chunk that is not live), and camera 5 still without an orientation
    behind n_filter.  Every solve starts with the heights alone (n = 3).
    The prior's weight is 1e-4: the solve of the step without edges takes six steps and stops by the gradient rule with
    the camera some 7e-3 rad from straight down - nearer than about 1e-3 rad the acos of PointsDownwardsPrior loses its
    digits in fp64 itself (tests/test_plane_eval_oracle.py, test_downward_prior_near_straight_down)."""
    S = Scene("bootstrap", seed, _cluster(6))
    S.cam_optimize[:] = [0, 1, 1, 1, 0, 0]
    S.cam_q[[3, 4, 5]] = np.nan
    S.edge(1, 0, 1)
    S.edge(0, 1, 63)
    S.edge(1, 2, 64)
    S.edge(2, 0, 65)
    S.edge(3, 1, 130)
    S.edge(2, 3, 7)
    S.edge(0, 2, 5, dead=True)
    S.edge(4, 2, 9)
    S.edge(3, 4, 6, homography=False)
    S.edge(4, 5, 4)  # behind every n_filter: camera 5 has no orientation
    S.step(3, 0, 0, prev_cam=2)
    S.step(4, 0, 9, prev_cam=3)
    S.step(4, 1, 9, prev_cam=1)
    S.step(0, 2, 9)
    return S


def tiles(n_opt, seed, name=None, **kw):
    """One mode-2 step over a grid of n_opt optimised cameras and a constant one, linked to their right and lower neighbours
    (every second link listed from the higher camera to the lower: cam_a > cam_b): n = 3 n_opt + 3."""
    n = n_opt + 1
    S = Scene(name or f"n{3 * n_opt + 3}", seed, _cluster(n), **kw)
    S.cam_optimize[n_opt // 2] = 0
    cols = int(np.ceil(np.sqrt(n)))
    k = 0
    for i in range(n):
        for j in (i + 1, i + cols):
            if j < n and (j != i + 1 or j % cols):
                S.edge(*((j, i) if k % 2 else (i, j)), 3 + k % 3)
                k += 1
    S.step(0, 2, len(S.edges))
    return S


def rough(seed=71):
    """n15's shape with matches 30 and 120 pixels off: nearly every block on the linear branch of the Huber loss, where the
    Gauss-Newton model overshoots once the radius has grown - the solve with cameras rejects steps on its way"""
    return tiles(4, seed, name="rough", noise=(30.0, 120.0))


def small12(seed=37):
    """the last small system, one step: two optimised cameras with blocks, one held by its prior alone (camera 4: no edge)
    and the heights; cameras 2 and 3 constant.  Camera 4 starts 0.3 rad from straight down and the prior's weight is 1e-5:
    the solve's growing steps (the radius triples with every accepted one) take it to some 0.03 rad, clear of where the
    prior's acos loses its digits (see bootstrap)."""
    S = Scene("n12", seed, _cluster(5), prior_weight=1e-5)
    S.cam_optimize[:] = [1, 1, 0, 0, 1]
    S.cam_q[4] = qmul(DOWN, axis_angle([0.6, 0.8, 0.0], 0.3))
    for a, b, k in ((0, 1, 5), (2, 1, 4), (2, 3, 6), (3, 0, 3)):
        S.edge(a, b, k)
    S.step(0, 2, 4)
    return S


def failing(seed=41):
    """plane_eval_fixtures.failing's block as the chain can meet it: a constant camera half a metre over the ground that looks
    along the ground (a quarter turn about x), and a match at its principal point - its ray runs parallel to the step's
    flat start plane and the intersection fails.  Reported in fail_bits of the first evaluation of both solves."""
    S = Scene("failing", seed, _cluster(4))
    S.cam_optimize[3] = 0
    for a, b, k in ((0, 1, 4), (1, 2, 4), (2, 0, 3)):
        S.edge(a, b, k)
    q = axis_angle([1, 0, 0], -np.pi / 2)  # the camera's z axis along world +y
    S.cam_pos[3] = (0.5, -3.0, 0.5)
    S.cam_q[3] = S.q_true[3] = q
    P = S.cam_pos[3] + 3.5 * qrot(q, np.array([0.0, 0.0, 1.0]))
    first = len(S.inliers)
    S.inliers.append((project_ld(S.q_true[0], S.cam_pos[0], P), MODEL10[1:3].copy(), next(S._scores)))
    S.edges.append(dict(cam_a=0, cam_b=3, n=1, first=first, flags=0, H=np.eye(3).reshape(-1)))
    S.step(0, 2, 4)
    return S


def tie(seed=43):
    """the hand-over: the second step's extra edge holds one match twice - two matches share the best score of a cell, the
    device leaves the step to the host's grid filter: status 1, steps_done 1, the poses of step 0 committed"""
    S = Scene("tie", seed, _cluster(4))
    S.cam_optimize[3] = 0
    for a, b, k in ((0, 1, 4), (1, 2, 5), (2, 3, 4)):
        S.edge(a, b, k)
    e = S.edge(3, 0, 3)
    S.inliers.append(S.inliers[-1])
    S.edges[e]["n"] += 1
    S.step(0, 2, 3)
    S.step(0, 2, 4)
    return S


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> scene: n = 3 (heights alone; and the step without edges), 6, 12 (the last small system), 15 (the first on
    the tile route), 63 (the augmented row is row 63 of tile 0), 66 (two tile columns: claim (1, 0) carries tile (1, 1)),
    129 (three columns, 43 cameras); a failing block; rejected steps"""
    out = [bootstrap(), small12(), tiles(4, 51), tiles(20, 52), tiles(21, 53), tiles(42, 54), failing(), rough()]
    return {s.name: s for s in out}


IDENTITY_SCENES = ("bootstrap", "n12", "n66")


# ---- the set-up of a step, restated --------------------------------------------------------------------------------------
def to_matrix(q):
    """Eigen::Quaternion::toRotationMatrix in its operation order"""
    tx, ty, tz = 2 * q[0], 2 * q[1], 2 * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def _closest(d1, o1, d2, o2):
    n11, n12, n22 = d1 @ d1, d1 @ d2, d2 @ d2
    denom = n11 * n22 - n12 * n12
    if not abs(denom) > 1e-9:
        return np.full(3, np.nan), np.nan
    off = o1 - o2
    od1, od2 = off @ d1, off @ d2
    t, s = (n12 * od2 - n22 * od1) / denom, (n11 * od2 - n12 * od1) / denom
    p1, p2 = o1 + d1 * t, o2 + d2 * s
    g = p1 - p2
    return (p1 + p2) * 0.5, (g @ g) * (1 if t >= 0 and s >= 0 else -1)


def setup_numpy(arr, rays, q, n_filter, tri=TRI):
    """gridFilterMatchesPerImage and the block list of the edges [0, n_filter) at the orientations q, in fp64 numpy: keep
    flags, the block lists (match indices inside the edge), the smallest relative gap between the best and the second
    score of a cell, and the smallest distance of a kept match's midpoint to the triangle's border test (both must be
    clear for the restatement to be the device's)."""
    edges, inl = arr["edges"], arr["inliers"]
    keep = np.zeros(len(inl), np.uint8)
    lists, gap_min, scores = [], np.inf, np.zeros(len(inl))
    ms = arr["models10"][0]
    for e in range(len(edges)):
        ed = edges[e]
        if e >= n_filter:
            lists.append(np.zeros(0, np.int64))
            continue
        a, b, first, k = int(ed["cam_a"]), int(ed["cam_b"]), int(ed["inlier_offset"]), int(ed["n_inliers"])
        Rs, Rd = to_matrix(q[a]), to_matrix(q[b])
        so, do = arr["cam_pos"][a], arr["cam_pos"][b]
        H = ed["H"]
        best = {}
        for i in range(k):
            m = inl[first + i]
            sd, dd = Rs @ rays[first + i, :3], Rd @ rays[first + i, 3:]
            _, gap = _closest(sd, so, dd, do)
            s = (0.0 if gap < 0 else 1.0 / (1.0 + gap)) * (1.0 - (sd @ dd) ** 2) * m["descriptor_score"]
            if ed["flags"] & 1:
                sx, sy = (m["px1"] - ms[1:3]) / ms[0]
                dx, dy = (m["px2"] - ms[1:3]) / ms[0]
                h = H.reshape(3, 3) @ np.array([sx, sy, 1.0])
                s = s * (1.0 / (1.0 + np.sqrt((dx - h[0] / h[2]) ** 2 + (dy - h[1] / h[2]) ** 2)))
            scores[first + i] = s
            if not s > 0:
                continue
            cells = (("s", int(np.floor(m["px1"][0] / ms[8] / GRID)), int(np.floor(m["px1"][1] / ms[9] / GRID))),
                     ("d", int(np.floor(m["px2"][0] / ms[8] / GRID)), int(np.floor(m["px2"][1] / ms[9] / GRID))))
            for c in cells:
                best.setdefault(c, []).append((s, i))
        for c, v in best.items():
            v.sort(reverse=True)
            keep[first + v[0][1]] |= 1 if c[0] == "s" else 2
            if len(v) > 1:
                gap_min = min(gap_min, (v[0][0] - v[1][0]) / v[0][0])
        blk = []
        for i in range(k):
            if not keep[first + i]:
                continue
            mid, _ = _closest(qrot(q[a], rays[first + i, :3]), so, qrot(q[b], rays[first + i, 3:]), do)
            t = np.asarray(tri).reshape(3, 2)
            ok = not np.isnan(mid[0])
            for j in range(3):
                bb, cc = t[j], t[(j + 1) % 3]
                ok = ok and not (bb[0] - mid[0]) * (cc[1] - mid[1]) - (bb[1] - mid[1]) * (cc[0] - mid[0]) < 0
            if ok:
                blk.append(i)
        lists.append(np.array(blk, np.int64))
    return dict(keep=keep, blk_idx=lists, score_gap=gap_min, scores=scores)


def step_numpy(arr, step, q, lists):
    """what after_setup / begin_step's shortcut and begin_solve derive from the block lists: counts, priors, cameras with
    blocks, live chunks, and cam_t of the solve with cameras (the heights-alone solve: all -1)"""
    edges = arr["edges"]
    n_cams = len(arr["cam_pos"])
    mode, cam = int(step["mode"]), int(step["cam"])
    opt = (np.arange(n_cams) == cam) if mode == 0 else arr["cam_optimize"].astype(bool)
    prior = opt & ~np.isnan(q).any(axis=1)
    blocks = np.zeros(n_cams, bool)
    n_live = 0
    cap_edge = 2 * int(np.ceil(1.0 / GRID)) ** 2
    for e, l in enumerate(lists):
        if len(l):
            blocks[[int(edges[e]["cam_a"]), int(edges[e]["cam_b"])]] = True
        cap = min(int(edges[e]["n_inliers"]), cap_edge)
        n_live += sum(1 for f in range(0, cap, 64) if f < len(l))
    active = opt & (blocks | prior)
    cam_t = np.where(active, 3 * (np.cumsum(active) - 1), -1)
    return dict(n_blocks=int(sum(len(l) for l in lists)), n_prior=int(prior.sum()), n_live=n_live, cam_prior=prior.astype(np.uint8),
                cam_blocks=blocks.astype(np.uint8), cam_t=cam_t, optimised=opt)


# ---- a traced evaluation as a plane problem ------------------------------------------------------------------------------
def plane_problem(arr, rays, lists, q, z, cam_t, cam_prior, which, tri=TRI):
    """the ochip_relax_desc fields (plane_eval_fixtures.to_relaxg takes them on) of the system an evaluation assembled: the
    blocks of the lists in edge order, the priors of the active cameras (a constant camera's prior is fixed cost, not in
    the reduced program), cameras with cam_t >= 0 optimised (which = 0: structure_only, no camera).  A camera without an
    orientation takes the identity: it has neither block nor prior."""
    edges = arr["edges"]
    a, b, r = [], [], []
    for e, l in enumerate(lists):
        for i in l:
            a.append(int(edges[e]["cam_a"]))
            b.append(int(edges[e]["cam_b"]))
            r.append(rays[int(edges[e]["inlier_offset"]) + int(i)])
    qq = np.array(q, float)
    qq[np.isnan(qq).any(axis=1)] = (0, 0, 0, 1)
    act = np.asarray(cam_t) >= 0
    return dict(cam_pos=arr["cam_pos"], cam_q=qq, cam_optimize=act.astype(np.uint8), plane_xy=np.asarray(tri, float),
                plane_z=np.asarray(z, float), z_optimize=np.ones(3, np.uint8), blk_cam_a=np.array(a, np.uint32),
                blk_cam_b=np.array(b, np.uint32), blk_rays=np.array(r, float).reshape(-1, 6),
                prior_cam=np.flatnonzero(np.asarray(cam_prior).astype(bool) & act).astype(np.uint32) if which else np.zeros(0, np.uint32),
                huber_a=HUBER_A, prior_weight=arr["prior_weight"])


def columns(ref_order, cam_t, n_active, nz, n_ref):
    """chain column of every canonical column of an oracle evaluation: camera c at cam_t[c], the heights behind the cameras"""
    n_cams = len(cam_t)
    perm = np.full(n_ref, -1)
    for c in range(n_cams):
        co = int(ref_order[c])
        assert (co >= 0) == (cam_t[c] >= 0), (c, co, cam_t[c])
        if co >= 0:
            perm[co:co + 3] = cam_t[c] + np.arange(3)
    for k in range(3):
        co = int(ref_order[n_cams + k])
        assert (co >= 0) == (nz > 0), (k, co, nz)
        if co >= 0:
            perm[co] = 3 * n_active + k
    assert np.all(perm >= 0) and len(set(perm)) == n_ref
    return perm


def eval_ratios(got_cost, got_A, got_g, ref, perm):
    """the worst error-to-bound ratios (relax_eval_fixtures.bounds, c = 2^18; the cost as the reduced program's) of an
    evaluation in the chain's column order (A: its lower triangle) against a long-double evaluation"""
    A = np.tril(got_A) + np.tril(got_A, -1).T
    red = dict(ref, cost=ref["cost_reduced"])
    return G.ratios(dict(cost=got_cost, JtJ=A[np.ix_(perm, perm)], Jtr=np.asarray(got_g)[perm]), red)


# ---- the linear solve ------------------------------------------------------------------------------------------------------
def jacobi_scale(d):
    return 1.0 / (1.0 + np.sqrt(d))


def clamp_diagonal(v):
    lo = np.where(v < 1e-6, 1e-6, v)
    return np.where(1e32 < lo, 1e32, lo)


def damping(diagonal, radius):
    dd = np.sqrt(diagonal / radius)
    return dd * dd


def system(A, g, scale, lm_diag):
    """(n + 1) x n: the lower triangle of S A S + D in the kernel's operation order ((a s_i) s_j, then the damping on the
    diagonal) and the scaled gradient as row n"""
    n = len(g)
    W = np.zeros((n + 1, n))
    W[:n] = np.tril((np.tril(A) * scale[:, None]) * scale[None, :])
    W[np.arange(n), np.arange(n)] += lm_diag
    W[n] = g * scale
    return W


def small_cholesky(W):
    """the one-thread factorisation and solves of start_iteration for n <= 12, in its operation order: (step, bad)"""
    n = W.shape[1]
    Wm, gs = W[:n].copy(), W[n]
    bad = False
    for j in range(n):
        d = Wm[j, j]
        for k in range(j):
            d -= Wm[j, k] * Wm[j, k]
        bad = bad or not d > 0
        l = np.sqrt(d) if d >= 0 else np.nan
        Wm[j, j] = l
        for i in range(j + 1, n):
            v = Wm[i, j]
            for k in range(j):
                v -= Wm[i, k] * Wm[j, k]
            Wm[i, j] = v / l
    y = np.zeros(n)
    for i in range(n):
        v = gs[i]
        for k in range(i):
            v -= Wm[i, k] * y[k]
        y[i] = v / Wm[i, i]
    for i in range(n - 1, -1, -1):
        v = y[i]
        for k in range(i + 1, n):
            v -= Wm[k, i] * y[k]
        y[i] = v / Wm[i, i]
    return y, bad


def model_ratio(gs, lm_diag, x, mcc):
    """lm_fixtures.model_ratio on the traced vectors"""
    n = len(x)
    xl, gl, dl = x.astype(LD), gs.astype(LD), lm_diag.astype(LD)
    m = LD(0.5) * np.sum(xl * gl + dl * xl * xl)
    s = LD(0.5) * np.sum(np.abs(xl * gl) + dl * xl * xl)
    return float(abs(LD(mcc) - m)) / (LM.C_MODEL * n * U * float(s))


def solve_ld(W):
    """the step of the system in long double (Cholesky)"""
    n = W.shape[1]
    A = LM.full(W).astype(LD)
    L = np.zeros((n, n), LD)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(n, LD)
    for i in range(n):
        y[i] = (LD(W[n, i]) - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n, LD)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def solve_ratios(W, x, mcc, lm_diag, L=None):
    """the ratios of a linear solve against lm_fixtures' componentwise bounds (constants 4): backward (the step) and model
    (mcc) on both routes; with the tile route's factor (L: (n + 1) x n with the augmented row y) also factor and forward;
    for a well-conditioned system (kappa < 1e4) forward_error against the long-double solve"""
    n = len(x)
    out = dict(backward=LM.backward_ratio(W, x), model=model_ratio(W[n], lm_diag, x, mcc))
    if L is not None:
        stored = np.tril(np.ones(((n + 63) // 64,) * 2, bool))
        out["factor"] = LM.factor_ratio(W, L[:n], stored)
        out["forward"] = LM.forward_ratio(L[:n], L[n], W[n])
    kap = LM.kappa(W)
    if kap < 1e4:
        out["forward_error"] = LM.forward_error_ratio(W, x, solve_ld(W).astype(np.float64), kap)
    return out


# ---- the candidate -----------------------------------------------------------------------------------------------------------
def candidate_ld(q, z, cam_t, n_active, nz, scale, x):
    """x (+) (-x_step scale) in long double: lm_quat_plus per camera with unknowns, z - step scale"""
    q = np.asarray(q, LD).copy()
    d_all = -(np.asarray(x, LD) * np.asarray(scale, LD))
    for c, tc in enumerate(cam_t):
        if tc < 0:
            continue
        d = d_all[tc:tc + 3]
        nrm = np.sqrt(d @ d)
        if nrm == 0:
            continue
        s = np.sin(nrm) / nrm
        q[c] = qmul(np.array([s * d[0], s * d[1], s * d[2], np.cos(nrm)]), q[c])
    zz = np.asarray(z, LD) + (d_all[3 * n_active:3 * n_active + 3] if nz else 0)
    return q, zz


# ---- relax_lm_rules.hpp: lm_trust and the termination rules, transcribed -----------------------------------------------------
OPTIONS = dict(max_num_iterations=100, initial_trust_region_radius=1.0, function_tolerance=1e-6, gradient_tolerance=1e-10,
               parameter_tolerance=1e-8)
(NO_CONVERGENCE, CONVERGENCE_FUNCTION, CONVERGENCE_GRADIENT, CONVERGENCE_PARAMETER, CONVERGENCE_RADIUS, FAILURE,
 NO_PARAMETERS) = ("no_convergence", "function", "gradient", "parameter", "radius", "failure", "no_parameters")


class Trust:
    def __init__(self, radius):
        self.radius, self.decrease, self.invalid = radius, 2.0, 0

    def on_invalid(self):
        self.invalid += 1
        if self.invalid >= 5:
            return True
        self.radius *= 0.5
        return False

    def on_accept(self, rho):
        t = 2.0 * rho - 1.0
        b = 1.0 - t * t * t
        self.radius = self.radius / (b if 1.0 / 3.0 < b else 1.0 / 3.0)
        self.radius = self.radius if self.radius < 1e16 else 1e16
        self.decrease = 2.0

    def on_reject(self):
        self.radius = self.radius / self.decrease
        self.decrease *= 2.0


def replay(first_eval, iterations):
    """The trust-region loop of the chain's serial part (after_asm, start_iteration) fed with the traced figures.
    first_eval: dict(cost, gmax, fail_bits, x_norm); iterations: per linear solve dict(mcc, chol_fail, step_norm, cand_norm,
    cost, gmax, fail_bits) of the candidate's evaluation.  Returns dict(termination, iterations, radii (the radius of every
    linear solve), accepted (per solve: True / False / None for an invalid step), used (solves consumed))."""
    o = OPTIONS
    out = dict(radii=[], accepted=[], used=0)

    def done(term, iters):
        out.update(termination=term, iterations=iters)
        return out

    if first_eval["fail_bits"]:
        return done(FAILURE, 0)
    trust = Trust(o["initial_trust_region_radius"])
    x_cost, x_norm, iters, it = first_eval["cost"], first_eval["x_norm"], 1, 0
    if first_eval["gmax"] <= o["gradient_tolerance"]:
        return done(CONVERGENCE_GRADIENT, iters)
    k = 0
    while True:
        if it >= o["max_num_iterations"]:
            return done(NO_CONVERGENCE, iters)
        if trust.radius <= 1e-32:
            return done(CONVERGENCE_RADIUS, iters)
        it += 1
        iters += 1
        s = iterations[k]
        k += 1
        out["used"] = k
        out["radii"].append(trust.radius)
        valid = not s["chol_fail"] and np.isfinite(s["mcc"]) and s["mcc"] > 0.0
        if not valid:
            out["accepted"].append(None)
            if trust.on_invalid():
                return done(FAILURE, iters)
            continue
        cand_cost = 1.7976931348623157e308 if s["fail_bits"] & 1 else s["cost"]
        trust.invalid = 0
        out["accepted"].append(False)
        if s["step_norm"] <= o["parameter_tolerance"] * (x_norm + o["parameter_tolerance"]):
            return done(CONVERGENCE_PARAMETER, iters)
        change = x_cost - cand_cost
        if abs(change) <= o["function_tolerance"] * x_cost:
            return done(CONVERGENCE_FUNCTION, iters)
        rho = change / s["mcc"]
        if rho > 1e-3:
            out["accepted"][-1] = True
            x_norm, x_cost = s["cand_norm"], s["cost"]
            trust.on_accept(rho)
            if s["fail_bits"] & 2:
                return done(FAILURE, iters)
            if s["gmax"] <= o["gradient_tolerance"]:
                return done(CONVERGENCE_GRADIENT, iters)
        else:
            trust.on_reject()

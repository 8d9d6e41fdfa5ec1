"""Small seeded problems of the points relax engine (ochip_relaxp_desc, as dicts of its fields: capi.relaxp_desc) for the
evaluation and step tests, and the bounds the device's and the fp64 oracle's results are held to against the long-double
oracle (oracle/relaxp_eval.cpp).  Data and arithmetic only; no device.

The evaluation quantities (cost, J'J, J'r) use the normwise bounds of relax_eval_fixtures with a block being an observation
(or the monotonicity block) and the same C_BOUND.  The step quantities have forms of their own, each with one constant
calibrated in tests/test_relaxp_eval_oracle.py (the fp64 oracle against the long-double one, fp64 within half):
  W (the reduced, scaled, damped system and its right-hand side), C_W:
      |dW_ij| <= s_i s_j B_ij + C_W u ([i = j] D2_i + sum_p kappa_p |w_ip|' |Mpp_p^-1| |w_jp|), B the J'J bound above (W
      inherits the evaluation's error), w_ip = M_cp the scaled coupling of column i with point p, kappa_p the 2-norm
      condition number of the damped point block; the right-hand side the same with B_i of J'r, b_p for w_jp;
  pt_d (the unscaled step of a point), C_D: |d pt_d|_2 <= C_D u kappa_p |delta_p|_2;
  the model cost change, C_M: C_M u kappa sum_i (|y_i b_i| + D2_i y_i^2) / 2, kappa the largest kappa_p;
  |dx|^2, C_N: C_N u kappa |dx|^2; |x|^2: C_N u (|x|^2 + 2 kappa |dx| |x|);
  the points' slope g_p . d_p (and its alpha2 rerun): sum_i (B_i |delta_i| + |g_i| C_D u kappa_p |delta_p|) with B the J'r bound;
  the backward error of a full step y in the scaled system, |b - M y|_inf / (|M|_inf |y|_inf + |b|_inf): C_B u."""
import numpy as np

import relax_eval_fixtures as G
from relax_fixtures import DOWN, axis_angle, qinv, qmul, qrot

U = G.U
C_BOUND = G.C_BOUND
MODEL = G.MODEL
HUBER_A = 10.0
# calibrated in tests/test_relaxp_eval_oracle.py (its docstring holds the measured ratios)
C_W = 2.0 ** 8
C_D = 2.0 ** 20
C_M = 2.0 ** 8
C_N = 2.0 ** 17
C_B = 2.0 ** 10


def project(q, pos, X, m):
    """image_from_3d of the camera-frame ray of X: the forward lens model m = f ppx ppy k1 k2 k3 p1 p2"""
    ray = qrot(qinv(q), np.asarray(X, float) - pos)
    u = ray[:2] / max(ray[2], 1e-3)
    r2 = u @ u
    rd = m[3] * r2 + m[4] * r2 ** 2 + m[5] * r2 ** 3
    d = np.array([(1 + rd) * u[i] + 2 * u[0] * u[1] * m[6 + i] + m[7 - i] * (r2 + 2 * u[i] ** 2) for i in range(2)])
    return d * m[0] + m[1:3]


class Builder:
    """cameras at height 10 looking down (0.03 rad of noise), groups of points on rough ground between two cameras, pixels
    with 0.5 px of noise (every fifth observation 15 px: the linear branch of the Huber loss), starting points off by 5 cm"""

    def __init__(self, seed, n_cams=5, spacing=4.0, model=MODEL, ring=False, true_model=None):
        self.rng = rng = np.random.default_rng(seed)
        if ring:
            ang = 2 * np.pi * np.arange(n_cams) / n_cams
            rad = spacing * n_cams / (2 * np.pi)
            self.cam = np.stack([rad * np.cos(ang), rad * np.sin(ang), np.full(n_cams, 10.0)], 1)
        else:
            cols = int(np.ceil(np.sqrt(n_cams)))
            self.cam = np.array([[(i % cols) * spacing, (i // cols) * spacing, 10.0] for i in range(n_cams)])
        self.q = np.array([qmul(DOWN, axis_angle(a / np.linalg.norm(a), 0.03)) for a in rng.normal(size=(n_cams, 3))])
        self.model = np.array(model, float)
        self.true_model = self.model if true_model is None else np.array(true_model, float)
        self.grp_cam, self.grp_n, self.X, self.px = [], [], [], []

    def point(self, a, b, X, X0=None, px_sigma=None):
        """one point of the group being built: pixels of the true X in cameras a and b plus noise, the start X0"""
        rng = self.rng
        for c in (a, b):
            sigma = (15.0 if (len(self.px) % 5 == 0) else 0.5) if px_sigma is None else px_sigma
            self.px.append(project(self.q[c], self.cam[c], X, self.true_model) + rng.normal(size=2) * sigma)
        self.X.append(np.asarray(X, float) + rng.normal(size=3) * 0.05 if X0 is None else np.asarray(X0, float))

    def group(self, a, b, k):
        self.grp_cam.append((a, b))
        self.grp_n.append(k)
        mid = (self.cam[a, :2] + self.cam[b, :2]) / 2
        for _ in range(k):
            self.point(a, b, [*(mid + self.rng.normal(size=2) * 1.5), self.rng.normal() * 0.3])

    def scene(self, functor=3, opt=(1, 1, 3), cam_optimize=None, mono=0, mono_r_max=0.0, huber_a=HUBER_A, **extra):
        n_cams = len(self.cam)
        s = dict(cam_pos=self.cam.copy(), cam_q=self.q.copy(),
                 cam_optimize=np.ones(n_cams, np.uint8) if cam_optimize is None else np.asarray(cam_optimize, np.uint8),
                 point_xyz=np.array(self.X, float).reshape(-1, 3),
                 grp_first=np.concatenate([[0], np.cumsum(self.grp_n)]).astype(np.uint32),
                 grp_cam=np.array(self.grp_cam, np.uint32).reshape(-1, 2), obs_px=np.array(self.px, float).reshape(-1, 2),
                 functor=functor, model=self.model.copy(), opt_focal=opt[0], opt_principal=opt[1], n_radial_free=opt[2],
                 focal_lo=100.0, focal_hi=20000.0, huber_a=huber_a, mono_observations=mono, mono_r_max=mono_r_max)
        s.update(extra)
        return s


PAIRS = [(0, 1), (1, 2), (2, 3), (3, 4), (0, 2)]


def functor(level, opt=(1, 1, 3), seed=None):
    """one functor level under one (opt_focal, opt_principal, n_radial_free): five cameras, five groups of 4 .. 6 points"""
    B = Builder(100 + 16 * level + 8 * opt[0] + 4 * opt[1] + opt[2] if seed is None else seed)
    for i, (a, b) in enumerate(PAIRS):
        B.group(a, b, 4 + i % 3)
    return B.scene(functor=level, opt=opt)


def roles(seed=131):
    """groups listed as (b, a) with b > a; camera 1 is side b of one group and side a of another; the constant camera 4 inside
    groups; the optimised camera 6 without a group; the optimised camera 5 whose only group is empty, that empty group
    between non-empty ones"""
    B = Builder(seed, n_cams=7)
    B.group(2, 1, 5)
    B.group(1, 3, 4)
    B.group(3, 4, 6)
    B.group(0, 5, 0)
    B.group(4, 0, 3)
    B.group(0, 2, 5)
    return B.scene(functor=3, cam_optimize=[1, 1, 1, 1, 0, 1, 1])


def sizes(seed=132):
    """groups of 1, 63, 64, 65 and 200 points (393: two blocks of point_kernel, a partial last block of obs_kernel, the
    strided loops of p_reduce and p_candidate past their 256 threads)"""
    B = Builder(seed, n_cams=6)
    for (a, b), k in zip([(0, 1), (2, 1), (1, 3), (3, 4), (4, 5)], (1, 63, 64, 65, 200)):
        B.group(a, b, k)
    return B.scene(functor=2, opt=(1, 1, 2))


def wide(seed=133):
    """24 optimised cameras in a ring, 3 .. 5 points per edge: 72 + 8 reduced unknowns, two 64-column blocks"""
    B = Builder(seed, n_cams=24, ring=True)
    for i in range(24):
        B.group(i, (i + 1) % 24, 3 + i % 3)
    return B.scene(functor=3)


def huber_edge(side, seed=134):
    """the observation nearest the threshold gets s = a^2 (1 + 1e-5) (side > 0: the linear branch) or a^2 (1 - 1e-5)"""
    from oracle import pyoracle

    s = functor(3, seed=seed)
    e = pyoracle.relaxp_eval(s, raw=True, jacobian=False)
    sq = np.bincount(e["row_blk"], weights=e["r"] ** 2)
    o = int(np.argmin(np.abs(np.log(sq / HUBER_A ** 2))))
    s["huber_a"] = float(np.sqrt(sq[o] / (1 + 1e-5 * side)))
    return s


def behind(seed=135):
    """the last point of the first group lies half a metre BEHIND camera 0 (camera-frame z = -0.5 < 1e-3: the clamp, no
    depth partial) and in front of camera 1, which is raised to 14 m"""
    B = Builder(seed)
    B.cam[1, 2] = 14.0
    B.grp_cam.append((0, 1))
    B.grp_n.append(4)
    mid = (B.cam[0, :2] + B.cam[1, :2]) / 2
    for _ in range(3):
        B.point(0, 1, [*(mid + B.rng.normal(size=2) * 1.5), B.rng.normal() * 0.3])
    X = B.cam[0] + qrot(B.q[0], np.array([2e-4, -1e-4, -0.5]))
    B.point(0, 1, X, X0=X, px_sigma=0.5)
    for a, b in PAIRS[1:]:
        B.group(a, b, 4)
    return B.scene(functor=0, opt=(0, 0, 0))


def far(seed=136):
    """the last point of the first group at depth 1e7: its diag S^2 is ~1e-8, below the 1e-6 floor of the damping's clamp"""
    B = Builder(seed)
    B.group(0, 1, 3)
    B.grp_n[-1] += 1
    X = np.array([2.0, 0.0, -1e7])
    B.point(0, 1, X, X0=X + np.array([3.0, -2.0, 50.0]), px_sigma=0.5)
    for a, b in PAIRS[1:]:
        B.group(a, b, 4)
    return B.scene(functor=1, opt=(1, 1, 0))


def mono_active(n_radial_free, seed=137):
    """1 + 3 k1 r^2 + 5 k2 r^4 is negative at the outer samples of r <= 1 and positive at the inner ones"""
    model = MODEL.copy()
    model[3:6] = [-0.5, 0.05, 0.0]
    B = Builder(seed + n_radial_free, model=model)
    for i, (a, b) in enumerate(PAIRS):
        B.group(a, b, 4 + i % 3)
    return B.scene(functor=2 if n_radial_free == 1 else 3, opt=(1, 1, n_radial_free), mono=40, mono_r_max=1.0)


def focal_bound(seed=138):
    """the pixels come from f = 1100, the state holds 1000 and focal_hi = 1000.5: the gradient-like step of radius 1e-2 moves
    f to 1000.92 and is clamped (the step of radius 1e4 follows the noise the other way and is not)"""
    true = MODEL.copy()
    true[0] = 1100.0
    B = Builder(seed, true_model=true)
    for i, (a, b) in enumerate(PAIRS):
        B.group(a, b, 6)
    return B.scene(functor=1, opt=(1, 1, 0), focal_hi=1000.5)


def failing(seed=139):
    s = functor(1, seed=seed)
    s["obs_px"][3, 1] = np.nan
    return s


def at_state(scene, cam_q, point_xyz, model):
    """the same problem at another state"""
    s = dict(scene)
    s.update(cam_q=np.array(cam_q, float), point_xyz=np.array(point_xyz, float).reshape(-1, 3), model=np.array(model, float))
    return s


_CASES = None


def cases():
    """(name, scene, structure_only)"""
    global _CASES
    if _CASES is None:
        out = [(f"functor{k}", functor(k), False) for k in range(4)]
        out += [(f"functor1_f{f}_pp{p}", functor(1, (f, p, 0)), False) for f, p in ((1, 0), (0, 1), (0, 0))]
        out += [(f"functor{k}_k{nk}", functor(k, (1, 1, nk)), False) for k in (2, 3) for nk in range(4)]
        out += [("roles", roles(), False), ("sizes", sizes(), False), ("wide", wide(), False),
                ("huber_above", huber_edge(+1), False), ("huber_below", huber_edge(-1), False), ("behind", behind(), False),
                ("far", far(), False), ("mono_active_k1", mono_active(1), False), ("mono_active_k3", mono_active(3), False),
                ("focal_bound", focal_bound(), False), ("roles_structure_only", roles(), True),
                ("functor3_structure_only", functor(3), True)]
        _CASES = out
    return _CASES


def case(name):
    return next((s, so) for n, s, so in cases() if n == name)


# ---- bounds ------------------------------------------------------------------------------------------------------------
def eval_bounds(ref, c=C_BOUND):
    """relax_eval_fixtures.bounds over all N columns of a relaxp_eval (a block = an observation or the monotonicity block)"""
    return G.bounds(dict(ref, n=ref["N"]), c)


def split_eval(e):
    """the parts of a full evaluation the device returns: U, g_c, per point V (xx xy xz yy yz zz) and g_p"""
    n, N = e["n"], e["N"]
    P = (N - n) // 3
    idx = n + 3 * np.arange(P)
    A = e["JtJ"]
    tri = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    V = np.stack([A[idx + a, idx + b] for a, b in tri], 1) if P else np.zeros((0, 6))
    return dict(U=A[:n, :n], g_c=e["Jtr"][:n], V=V, g_p=e["Jtr"][n:].reshape(-1, 3))


def eval_ratios(got, ref, b=None):
    """worst error-to-bound ratios of cost, U, g_c, V, g_p and the point-gradient maximum.  got: cost, U, g_c (canonical
    order), V, g_p, gmax_p; ref: a long-double relaxp_eval"""
    b = eval_bounds(ref) if b is None else b
    r, rb = split_eval(ref), split_eval(dict(ref, JtJ=b["JtJ"], Jtr=b["Jtr"]))
    out = dict(cost=G.ratio(got["cost"] - ref["cost"], b["cost"]))
    for k in ("U", "g_c", "V", "g_p"):
        out[k] = G.ratio(np.asarray(got[k]) - r[k], rb[k])
    gm = np.max(np.abs(r["g_p"])) if r["g_p"].size else 0.0
    out["gmax_p"] = G.ratio(got["gmax_p"] - gm, np.max(rb["g_p"]) if r["g_p"].size else 0.0)
    return out


def point_cond(step):
    """2-norm condition number of every damped point block of a reference step"""
    return np.array([np.linalg.cond(m) for m in step["Mpp"]]) if len(step["Mpp"]) else np.zeros(0)


def step_bounds(ref, step, eb=None):
    """the bounds of the step quantities (the head of this file) from a long-double evaluation and step"""
    eb = eval_bounds(ref) if eb is None else eb
    n, N = ref["n"], ref["N"]
    P = (N - n) // 3
    s, D2, y, b, delta = step["scale"], step["D2"], step["y"], ref["Jtr"] * step["scale"], step["delta"]
    kap = point_cond(step)
    kmax = float(np.max(kap)) if P else 1.0
    We = s[:n, None] * s[None, :n] * eb["JtJ"][:n, :n]
    re = s[:n] * eb["Jtr"][:n]
    Wb, rb = np.diag(D2[:n]), np.zeros(n)
    if P and n:
        Mcp = (ref["JtJ"][:n, n:] * s[:n, None] * s[None, n:]).reshape(n, P, 3)
        Minv = np.abs(np.linalg.inv(step["Mpp"]))  # P x 3 x 3
        t = np.einsum("ipa,pab->ipb", np.abs(Mcp), Minv) * kap[None, :, None]
        Wb = Wb + np.einsum("ipb,jpb->ij", t, np.abs(Mcp))
        rb = rb + np.einsum("ipb,pb->i", t, np.abs(b[n:].reshape(P, 3)))
    dn = np.linalg.norm(delta[n:].reshape(P, 3), axis=1) if P else np.zeros(0)
    ptd = C_D * U * kap * dn
    terms = 0.5 * np.sum(np.abs(y * b) + D2 * y * y)
    slope_p = float(np.sum(eb["Jtr"][n:] * np.abs(delta[n:])) + np.sum(np.abs(ref["Jtr"][n:]).reshape(P, 3) * ptd[:, None]))
    return dict(W=We + C_W * U * Wb, rhs=re + C_W * U * rb, pt_d=ptd, kappa=kap, model_cost_change=C_M * U * kmax * terms,
                step_sq=C_N * U * kmax * step["step_sq"],
                cand_sq=C_N * U * (step["cand_sq"] + 2 * kmax * np.sqrt(step["step_sq"] * step["cand_sq"])),
                slope_p=slope_p, backward_error=C_B * U)


def step_ratios(got, ref, step, sb=None):
    """worst error-to-bound ratios of a step against the reference.  got: optional W ((n + 1) x n lower triangle, row n the
    right-hand side; canonical order), pt_d, model_cost_change, step_sq, cand_sq, slope_p"""
    sb = step_bounds(ref, step) if sb is None else sb
    n, N = ref["n"], ref["N"]
    out = {}
    if got.get("W") is not None and n:
        lo = np.tril(np.ones((n, n), bool))
        out["W"] = G.ratio((got["W"][:n] - step["Sc"])[lo], sb["W"][lo])
        out["rhs"] = G.ratio(got["W"][n] - step["rhs_c"], sb["rhs"])
    if got.get("pt_d") is not None and N > n:
        err = np.linalg.norm(np.asarray(got["pt_d"]) - step["delta"][n:].reshape(-1, 3), axis=1)
        out["pt_d"] = G.ratio(err, sb["pt_d"])
    for k in ("model_cost_change", "step_sq", "cand_sq", "slope_p"):
        if got.get(k) is not None:
            out[k] = G.ratio(got[k] - step[k], sb[k])
    return out


STATE_TOL = 16 * U  # a candidate's coordinate from the same step: a product, sin / cos and a four-term sum of roundings


def state_bound(x2, dx_bound=0.0):
    """|candidate coordinate| error: STATE_TOL relative to max(1, |x2|) plus what the step itself may be off by"""
    return STATE_TOL * np.maximum(1.0, np.abs(x2)) + dx_bound

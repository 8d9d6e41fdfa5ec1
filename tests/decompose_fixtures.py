"""Homographies with a known motion for homography_model::decompose (cv::decomposeHomographyMat(H, I), the cheirality vote
over the inlier rays, std::stable_sort with `score >=`; csrc/decompose.hpp, oracle/ransac.cpp), the rays of the vote, and
what the returned poses are held to.  Data and arithmetic only; numpy, deterministic, no device.

Every H is built in 80-bit long double as s (R + (t/d) n^T) and rounded to fp64 once; the case keeps the truth (R, t/d, n,
s).  Nothing here restates the analytical decomposition: the expected values come from the truth and from the returned poses
alone (check_poses below) -
  rotation  every R(q) is a rotation (|q| = 1, det > 0)
  twins     two distinct rotations, each twice, the translation negated bit for bit between the twins
  truth     one pose is (R, +-t/d)
  rank one  with Hn = +-H / sigma_2 (numpy.linalg.svd in fp64: 1e-16 against an error floor of 1e-8) every pose has
            Hn - R_i = t_i n_i^T with n_i := (Hn - R_i)^T t_i / |t_i|^2 and |n_i| = 1
  votes     score_i = the number of flagged rays with n_i . a >= 0 and (R_i n_i) . b >= 0
  order     score descending, equal scores in descending solution index (tests/decompose_order_driver.cpp proves that this
            is what libstdc++'s std::stable_sort leaves with the non-strict comparator)

The error model.  v = 2 sqrtf(1 + tr S - M00 - M11 - M22) is single precision in the reference (OpenCV calls sqrtf) and the
port keeps it; |t|^2 = 2 + tr S - v then cancels, so with tau = |t| / d the poses are good to about 2^-24 / tau^2 only.
gamma = 1 + n^T R^T t / d = det(R + t n^T / d) is the ratio of the plane's depths in the two cameras (valid motions: > 0).
    E = C_DEC 2^-24 / (min(1, tau^2) gamma) + C_DEC 2^-53 kappa(H)
bounds |R(q) - R|, |t_out -+ t/d| / max(tau, 1), the rank-one residual and | |q| - 1 |.  An exact rotation (tau = 0) never
reaches the square root - the pure-rotation shortcut returns H / sigma_2 - and is held to the second term alone.
C_DEC: calibrated in tests/test_decompose_oracle.py (its docstring and DESIGN.md section 2 carry the measured ratios).

The S, minors, branch and signs below are computed from the truth in long double, for the coverage assertions and for the
classification only."""
import functools
import json

import numpy as np

from homography_fit_fixtures import LD, UNIT, rays_of

U24 = 2.0 ** -24
U = 2.0 ** -53
C_DEC = 2.0 ** 3         # calibration: tests/test_decompose_oracle.py
EPSILON = 0.001          # the pure-rotation threshold on max |S_ij|
GAMMA_MIN = 0.05
ZERO = 1e-12             # a quantity of the truth below this (relative to |S| of its degree) counts as a zero
MARGIN = 1e-6            # a ray of the vote keeps this distance from every plane it is counted against


# ------------------------------------------------------------------------------------------------------- rotations
def rotation(axis, angle):
    """Rodrigues in long double"""
    a = np.asarray(axis, LD)
    a = a / np.sqrt(np.sum(a * a))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], LD)
    ang = LD(angle)
    return np.eye(3, dtype=LD) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def yaw90(k):
    """the exact rotation by k x 90 degrees about z"""
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][k % 4]
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], LD)


def rotation_of_quaternion(q):
    """R(q) of a unit quaternion x y z w, in long double, without normalising: a q off the unit sphere shows"""
    x, y, z, w = [LD(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], LD)


def unit(v):
    v = np.asarray(v, LD)
    return v / np.sqrt(np.sum(v * v))


# ------------------------------------------------------------------------------------------- the truth, classified
def _opp_minor(S, row, col):
    x1, x2 = (1 if col == 0 else 0), (1 if col == 2 else 2)
    y1, y2 = (1 if row == 0 else 0), (1 if row == 2 else 2)
    return S[y1, x2] * S[y2, x1] - S[y1, x1] * S[y2, x2]


def truth_facts(R, t, n):
    """S = A^T A - I of A = R + t n^T in long double: max |S_ij|, the branch (largest |S_ii|), the sign each branch reads
    (e12, e02, e01), and whether a zero of the truth decides something the result depends on: the sign of S_ii, the sign
    of the branch's minor, or the sign of a minor under a square root (a minor that is 0 in truth rounds to either side,
    and the negative side is a NaN)"""
    A = R + np.outer(t, n)
    S = A.T @ A - np.eye(3, dtype=LD)
    ninf = np.max(np.abs(S))
    d = [abs(S[i, i]) for i in range(3)]
    idx = 0
    if d[0] < d[1]:
        idx = 1
        if d[1] < d[2]:
            idx = 2
    elif d[0] < d[2]:
        idx = 2
    e_minor = [_opp_minor(S, 1, 2), _opp_minor(S, 0, 2), _opp_minor(S, 0, 1)][idx]
    roots = [(_opp_minor(S, 2, 2), _opp_minor(S, 1, 1)), (_opp_minor(S, 2, 2), _opp_minor(S, 0, 0)),
             (_opp_minor(S, 1, 1), _opp_minor(S, 0, 0))][idx]
    shortcut = bool(ninf < EPSILON)
    zero = False
    if not shortcut:
        zero = bool(abs(S[idx, idx]) <= ZERO * ninf or abs(e_minor) <= ZERO * ninf * ninf or
                    any(abs(m) <= ZERO * ninf * ninf for m in roots))
    return dict(S=S, ninf=float(ninf), idx=idx, e_sign=1 if e_minor >= 0 else -1, shortcut=shortcut, zero_decides=zero,
                near_threshold=bool(abs(ninf - EPSILON) <= 1e-9 * EPSILON))


def case(family, name, R, t, n, s=1.0, normalise22=False):
    """one homography with its truth.  t is t/d.  normalise22: the scale that makes H[2][2] = 1, as RANSAC delivers it"""
    R, t, n = np.asarray(R, LD), np.asarray(t, LD), np.asarray(n, LD)
    A = R + np.outer(t, n)
    if normalise22:
        s = 1 / A[2, 2]
    H = (LD(s) * A).astype(np.float64)
    tau = float(np.sqrt(np.sum(t * t)))
    gamma = float(1 + n @ (R.T @ t))
    sv = np.linalg.svd(A.astype(np.float64), compute_uv=False)
    f = truth_facts(R, t, n)
    valid = gamma >= GAMMA_MIN
    c = dict(family=family, name=name, H=H, R=R, t=t, n=n, s=float(s), tau=tau, gamma=gamma, kappa=float(sv[0] / sv[2]),
             valid=valid, facts=f, solutions=1 if f["shortcut"] else 4)
    # The pure-rotation shortcut returns H / sigma_2 as it is (OpenCV does, and the port keeps it): under a negative scale
    # that is -R, which is no rotation, and its quaternion means nothing.  Past the shortcut the determinant is put right.
    c["improper"] = bool(f["shortcut"] and c["s"] < 0)
    c["bounded"] = bool(valid and not f["near_threshold"] and not f["zero_decides"] and not c["improper"])
    return c


def bound(c, C=C_DEC):
    """E of a bounded case"""
    if c["tau"] == 0:
        return C * U * c["kappa"]
    return C * U24 / (min(1.0, c["tau"] ** 2) * c["gamma"]) + C * U * c["kappa"]


# ------------------------------------------------------------------------------------------------------ the families
N_GENERAL = 480


def _draw_sphere(rng):
    return unit(rng.standard_normal(3))


@functools.lru_cache(None)
def general():
    """rotation angle 0 to pi about random axes, n over the whole sphere, tau log-uniform over [1e-3, 3], s = +-10^k for k in
    -8 .. 8, valid only"""
    rng = np.random.default_rng(8300)
    out = []
    while len(out) < N_GENERAL:
        i = len(out)
        R = rotation(_draw_sphere(rng), rng.uniform(0, np.pi))
        n = _draw_sphere(rng)
        tau = 10 ** rng.uniform(-3, np.log10(3))
        t = LD(tau) * _draw_sphere(rng)
        if 1 + n @ (R.T @ t) < GAMMA_MIN:
            continue
        s = (-1) ** (i // 17) * 10.0 ** (i % 17 - 8)
        out.append(case("general", "general%d" % i, R, t, n, s))
    return out


DRONE_KINDS = ("yaw_level", "yaw90", "identity_rotation", "climb", "t_perp_n", "h22_one")
LEVEL = np.array([0, 0, 1], LD)   # a level plane under a nadir camera


@functools.lru_cache(None)
def drone():
    """the survey's own motions, which put exact zeros into S"""
    rng = np.random.default_rng(8301)
    out = []

    def add(kind, R, t, n, **kw):
        out.append(case("drone", "%s%d" % (kind, sum(c["kind"] == kind for c in out)), R, t, n, **kw))
        out[-1]["kind"] = kind

    for k in range(8):   # yaw only over a level plane, translation in the plane
        add("yaw_level", rotation([0, 0, 1], rng.uniform(-np.pi, np.pi)), [rng.uniform(-1, 1), rng.uniform(-1, 1), 0], LEVEL)
    for k in range(4):   # yaw at exact multiples of 90 degrees: a drawn in-plane translation, and one along an axis
        add("yaw90", yaw90(k), [rng.uniform(0.1, 1), rng.uniform(0.1, 1), 0], LEVEL)
        add("yaw90", yaw90(k), [0.5, 0, 0], LEVEL)
    for k in range(6):   # R = I, t != 0
        add("identity_rotation", np.eye(3, dtype=LD), LD(10 ** rng.uniform(-2, 0)) * _draw_sphere(rng),
            LEVEL if k < 2 else _draw_sphere(rng))
    for k in range(6):   # pure climb: t parallel to n (in the first camera's frame: R^T t = h n)
        R = yaw90(0) if k == 0 else rotation([0, 0, 1], rng.uniform(-np.pi, np.pi)) if k < 3 else rotation(_draw_sphere(rng), rng.uniform(0, 1))
        n = LEVEL if k < 3 else _draw_sphere(rng)
        add("climb", R, R @ (LD(rng.uniform(0.1, 0.8)) * n), n)
    for k in range(6):   # t perpendicular to n (R^T t in the plane): gamma = 1
        R = rotation(_draw_sphere(rng), rng.uniform(0, 1))
        n = LEVEL if k < 2 else _draw_sphere(rng)
        p = np.cross(n, _draw_sphere(rng))
        add("t_perp_n", R, R @ (LD(rng.uniform(0.05, 1)) * unit(p)), n)
    for k in range(8):   # near-nadir motions scaled to H[2][2] = 1
        R = rotation([0, 0, 1], rng.uniform(-np.pi, np.pi)) @ rotation([rng.uniform(-1, 1), rng.uniform(-1, 1), 0], rng.uniform(0, 0.2))
        n = unit([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), 1])
        add("h22_one", R, [rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.3, 0.3)], n, normalise22=True)
    return out


def _tau_for(R, direction, n, target):
    """tau with max |S_ij| of R + tau direction n^T equal to target (max |S| grows with tau on the bracket), in long double"""
    lo, hi = LD(0), LD(1)
    for _ in range(200):
        mid = (lo + hi) / 2
        if np.max(np.abs(truth_facts(R, mid * direction, n)["S"])) < target:
            lo = mid
        else:
            hi = mid
    return hi


@functools.lru_cache(None)
def threshold():
    """tau chosen so that max |S_ij| lands at 0.001 (1 +- 10^-k), k = 1 .. 6, and exact rotations"""
    rng = np.random.default_rng(8302)
    out = []
    for k in range(1, 7):
        for side in (-1, 1):
            R = rotation(_draw_sphere(rng), rng.uniform(0, np.pi))
            n, d = _draw_sphere(rng), _draw_sphere(rng)
            tau = _tau_for(R, d, n, LD(EPSILON) * (1 + side * LD(10) ** -k))
            c = case("threshold", "threshold_%s_1e-%d" % ("below" if side < 0 else "above", k), R, tau * d, n)
            assert c["facts"]["shortcut"] == (side < 0) and abs(c["facts"]["ninf"] / (EPSILON * (1 + side * 10.0 ** -k)) - 1) < 1e-12
            out.append(c)
    zero = np.zeros(3, LD)
    out.append(case("threshold", "rotation_identity", np.eye(3, dtype=LD), zero, LEVEL))
    out.append(case("threshold", "rotation_minus_identity", np.eye(3, dtype=LD), zero, LEVEL, s=-1.0))
    for k in range(4):
        out.append(case("threshold", "rotation%d" % k, rotation(_draw_sphere(rng), rng.uniform(0, np.pi)), zero, LEVEL,
                        s=(1.0, -1.0, 1e-8, -1e8)[k]))
    out.append(case("threshold", "rotation_yaw90", yaw90(1), zero, LEVEL))
    out.append(case("threshold", "rotation_pi", yaw90(2), zero, LEVEL, s=3.0))
    return out


def motions():
    return general() + drone() + threshold()


@functools.lru_cache(None)
def degenerate():
    """agreement only: no motion stands behind these"""
    rng = np.random.default_rng(8303)
    g = general()[40]["H"] / general()[40]["s"]
    u, v, w = rng.standard_normal(3), rng.standard_normal(3), rng.standard_normal(3)
    nan, inf = g.copy(), g.copy()
    nan[1, 2] = np.nan
    inf[2, 0] = np.inf
    first_nan = g.copy()
    first_nan[0, 0] = np.nan
    out = [("zero", np.zeros((3, 3))), ("minus_zero", -np.zeros((3, 3))), ("rank1", np.outer(u, v)),
           ("rank2", np.outer(u, v) + np.outer(w, u)), ("rank2_diag", np.diag([2.0, 1.0, 0.0])),
           ("reflection", g @ np.diag([1.0, 1.0, -1.0])), ("reflection_diag", np.diag([1.0, 1.0, -1.0])),
           ("nan_entry", nan), ("nan_first", first_nan), ("all_nan", np.full((3, 3), np.nan)), ("inf_entry", inf),
           ("minus_inf_entry", -inf), ("x1e150", g * 1e150), ("x1e-150", g * 1e-150), ("x1e160", g * 1e160), ("x1e-170", g * 1e-170),
           ("mixed_1e150", g * np.array([[1e150], [1.0], [1e-150]])), ("denormal", g * 1e-310)]
    return [dict(family="degenerate", name="degenerate_" + k, H=np.ascontiguousarray(H, np.float64), bounded=False, valid=False,
                 solutions=None) for k, H in out]


# a few generic ray pairs every motion and degenerate job votes with (pixels of the unit model, so that the device can make
# the same rays): the vote and the order run on every H, bit for bit between the routes
def common_pixels():
    rng = np.random.default_rng(8304)
    return rng.uniform(-0.8, 0.8, (7, 2)), rng.uniform(-0.8, 0.8, (7, 2))


# ----------------------------------------------------------------------------------------------------------- the votes
def solution_from_normal(A, n):
    """the motion R + t n^T = A that belongs to the plane normal n: A agrees with R on the plane n^T x = 0"""
    e1 = unit(np.cross(n, [1, 0, 0] if abs(n[0]) < 0.9 else [0, 1, 0]))
    e2 = np.cross(n, e1)
    B = np.stack([e1, e2, n], 1)
    a1, a2 = A @ e1, A @ e2
    R = np.stack([a1, a2, np.cross(a1, a2)], 1) @ B.T
    return R, (A - R) @ n


def both_solutions(c):
    """the truth and the other motion with A = R + t n^T (up to the common sign of t and n), found without the analytical
    method: the plane normals are the two unit vectors n with |A x| = |x| on all of n^T x = 0, v2 x (a v1 +- b v3) of A's
    right singular vectors; each candidate is verified (R a rotation, A - R = t n^T) before it is used"""
    A = c["R"] + np.outer(c["t"], c["n"])
    _, sv, Vt = np.linalg.svd(A.astype(np.float64))
    v1, v2, v3 = [Vt[i].astype(LD) for i in range(3)]
    a, b = np.sqrt(LD(1 - sv[2] ** 2)), np.sqrt(LD(sv[0] ** 2 - 1))
    out = []
    for sign in (1, -1):
        n = unit(np.cross(v2, a * v1 + sign * b * v3))
        R, t = solution_from_normal(A, n)
        assert np.max(np.abs(R.T @ R - np.eye(3))) < 1e-12 and np.linalg.det(R.astype(np.float64)) > 0
        assert np.max(np.abs(R + np.outer(t, n) - A)) < 1e-12
        out.append((R, t, n))
    d = [min(np.max(np.abs(n - c["n"])), np.max(np.abs(n + c["n"]))) for _, _, n in out]
    assert min(d) < 1e-12 < max(d), d
    other = out[int(np.argmax(d))]
    return (c["R"], c["t"], c["n"]), other


@functools.lru_cache(None)
def vote_motion():
    """the fixed motion of the votes: a plane tilted 55 degrees against the optical axis, so that pixels see both sides of it"""
    R = rotation([0.3, -0.5, 0.8], 0.4)
    n = unit([np.sin(LD(55) * np.pi / 180), 0, np.cos(LD(55) * np.pi / 180)])
    c = case("votes", "vote_motion", R, [0.3, -0.2, 0.25], n)
    assert c["bounded"] and c["solutions"] == 4
    return c


def _sides(c, r1, r2):
    """per ray pair the four dot products against (n, R n) of the truth and of the other solution, in long double"""
    (R, _, n), (Rb, _, nb) = both_solutions(c)
    a, b = r1.astype(LD), r2.astype(LD)
    return np.stack([a @ n, b @ (R @ n), a @ nb, b @ (Rb @ nb)], 1)


@functools.lru_cache(None)
def ray_pool():
    """pixel pairs (unit model) by what they vote for: F = the truth and the other solution's visible side (real points on
    the plane, seen by both cameras), B = the twins of both (the ray of the first camera meets the plane behind it), X = the
    truth and the other solution's twin, Y = the truth's twin and the other solution (pairs that belong to no point), and
    NaN = a NaN coordinate.  Every pair keeps MARGIN from all four planes."""
    c = vote_motion()
    rng = np.random.default_rng(8305)
    A = (c["R"] + np.outer(c["t"], c["n"]))
    p1 = rng.uniform(-2.5, 2.5, (6000, 2))
    a = np.concatenate([p1, np.ones((len(p1), 1))], 1).astype(LD)
    X = a / (a @ c["n"])[:, None]          # the point of the plane on the ray (behind the camera where n . a < 0)
    Xp = X @ A.T
    real = (Xp / Xp[:, 2:3])[:, :2].astype(np.float64)
    p2 = np.where((np.arange(len(p1)) % 2 == 0)[:, None], real, rng.uniform(-2.5, 2.5, (len(p1), 2)))
    ok = np.all(np.abs(p2) < 50, 1)
    p1, p2 = p1[ok], p2[ok]
    d = _sides(c, rays_of(p1, UNIT), rays_of(p2, UNIT))
    keep = np.all(np.abs(d) >= MARGIN, 1)
    p1, p2, d = p1[keep], p2[keep], d[keep]
    sg = d > 0
    classes = dict(F=sg[:, 0] & sg[:, 1] & sg[:, 2] & sg[:, 3], B=~sg[:, 0] & ~sg[:, 1] & ~sg[:, 2] & ~sg[:, 3],
                   X=sg[:, 0] & sg[:, 1] & ~sg[:, 2] & ~sg[:, 3], Y=~sg[:, 0] & ~sg[:, 1] & sg[:, 2] & sg[:, 3])
    classes["none"] = ~(classes["F"] | classes["B"] | classes["X"] | classes["Y"])
    pool = {k: (p1[m], p2[m]) for k, m in classes.items()}
    for k in "FBXY":
        assert len(pool[k][0]) >= 40, (k, len(pool[k][0]))
    nan1, nan2 = p1[:30].copy(), p2[:30].copy()
    nan1[0::3, 0] = np.nan
    nan2[1::3, 1] = np.nan
    nan1[2::3, 1] = np.nan
    pool["NaN"] = (nan1, nan2)
    return pool


def _take(mix, M, seed):
    """M pixel pairs cycling through the classes of mix, shuffled"""
    pool = ray_pool()
    rng = np.random.default_rng(seed)
    px1, px2 = np.zeros((M, 2)), np.zeros((M, 2))
    for i in range(M):
        a, b = pool[mix[i % len(mix)]]
        px1[i], px2[i] = a[(i // len(mix)) % len(a)], b[(i // len(mix)) % len(b)]
    order = rng.permutation(M)
    px1, px2 = px1[order], px2[order]
    return px1, px2


VOTE_SIZES = (0, 1, 63, 64, 65, 127, 128, 129, 1000)
VOTE_FLAGS = ("none", "all", "last", "last_chunk", "every64th")


def _flags(kind, M):
    f = np.zeros(M, np.uint8)
    if kind == "all":
        f[:] = 1
    elif kind == "last":
        f[M - 1:] = 1
    elif kind == "last_chunk":   # those of the last partial chunk of 64 (the whole last chunk where M is a multiple)
        f[(M - 1) // 64 * 64 if M else 0:] = 1
    elif kind == "every64th":
        f[63::64] = 1
    return f


@functools.lru_cache(None)
def votes():
    """jobs of the vote: dict(name, case, px1, px2, flags).  The size x flags grid on a mix of every class; rows of one class
    alone and of all four in equal parts (the tie patterns - which of (n, 0, n, 0), (n, 0, 0, n), (0, n, n, 0), (0, n, 0, n)
    each is depends on the solution order of the decomposition: the four single-class rows realise all four); the same on a
    pure rotation, where N = 0 lets every flagged ray without a NaN vote"""
    c = vote_motion()
    rot = [m for m in threshold() if m["name"] == "rotation0"][0]
    out = []
    for M in VOTE_SIZES:
        for kind in VOTE_FLAGS:
            px1, px2 = _take(("F", "B", "F", "X", "NaN", "Y", "F", "none"), M, 100 + M)
            out.append(dict(name="votes_M%d_%s" % (M, kind), case=c, px1=px1, px2=px2, flags=_flags(kind, M), mix="grid"))
    for mix in ("F", "B", "X", "Y", "FBXY", "none", "NaN", "FX", "FB"):
        for M in (40, 65):
            px1, px2 = _take(tuple(mix) if mix not in ("none", "NaN") else (mix,), M, 200 + M)
            out.append(dict(name="votes_only_%s_M%d" % (mix, M), case=c, px1=px1, px2=px2, flags=_flags("all", M), mix=mix))
    for M in (0, 1, 64, 65, 129):
        for kind in ("all", "none", "last"):
            px1, px2 = _take(("F", "NaN", "B", "X"), M, 300 + M)
            out.append(dict(name="votes_rotation_M%d_%s" % (M, kind), case=rot, px1=px1, px2=px2, flags=_flags(kind, M), mix="rotation"))
    return out


def job_rays(j):
    return rays_of(j["px1"], UNIT), rays_of(j["px2"], UNIT)


# ------------------------------------------------------------------------------------------- what the poses are held to
def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.tobytes() == b.tobytes() or (np.array_equal(a, b, equal_nan=True) and
                                          np.array_equal(np.signbit(a[~np.isnan(a)]), np.signbit(b[~np.isnan(b)])))


def normalised(H):
    """+-H / sigma_2 in long double, the sign that makes the determinant positive"""
    sv = np.linalg.svd(H, compute_uv=False)
    Hn = H.astype(LD) / LD(sv[1])
    return -Hn if np.linalg.det(H / sv[1]) < 0 else Hn


def pose_planes(H, poses):
    """per returned pose (R_i, t_i, n_i, residual): n_i := (Hn - R_i)^T t_i / |t_i|^2 and the largest entry of
    Hn - R_i - t_i n_i^T; a pose without translation (the pure-rotation shortcut) has n_i = 0"""
    Hn = normalised(H)
    out = []
    for p in poses:
        if np.isnan(p[:7]).any():
            out.append(None)
            continue
        R, t = rotation_of_quaternion(p[:4]), p[4:7].astype(LD)
        tt = np.sum(t * t)
        n = (Hn - R).T @ t / tt if tt > 0 else np.zeros(3, LD)
        out.append((R, t, n, float(np.max(np.abs(Hn - R - np.outer(t, n))))))
    return out


def expected_scores(H, poses, r1, r2, flags):
    """the cheirality votes of the returned poses over the flagged rays, from the poses themselves"""
    a, b, f = r1.astype(LD), r2.astype(LD), np.asarray(flags, bool)
    out = []
    for pl in pose_planes(H, poses):
        if pl is None:
            out.append(-1)
            continue
        R, _, n, _ = pl
        with np.errstate(invalid="ignore"):
            out.append(int(np.sum(f & (a @ n >= 0) & (b @ (R @ n) >= 0))) if len(a) else 0)
    return out


def check_poses(c, poses, C=C_DEC):
    """a bounded case's four poses against the truth: (problems, ratios).  ratios: error / E per quantity (q = | |q| - 1 |,
    R and t of the pose nearest the truth, rank1 = the rank-one residual and | |n_i| - 1 |)"""
    E = bound(c, C)
    problems, ratios = [], {}
    present = [k for k in range(4) if not np.isnan(poses[k][:7]).any()]
    if len(present) != c["solutions"] or any(np.isnan(poses[k][:7]).all() != (k not in present) for k in range(4)):
        return ["%d solutions, %d expected" % (len(present), c["solutions"])], ratios
    planes = pose_planes(c["H"], poses)
    qn = [abs(float(np.sqrt(np.sum(poses[k][:4].astype(LD) ** 2))) - 1) for k in present]
    ratios["q"] = max(qn) / E
    for k in present:
        if not np.linalg.det(planes[k][0].astype(np.float64)) > 0:
            problems.append("pose %d: det R(q) <= 0" % k)
    if c["solutions"] == 4:
        # twins: a perfect matching into two pairs of equal q and negated t, the two rotations distinct
        pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)
                 if _same_bits(poses[i][:4], poses[j][:4]) and _same_bits(poses[i][4:7], -poses[j][4:7])]
        if len(pairs) != 2 or len({k for p in pairs for k in p}) != 4:
            problems.append("twins: %s" % pairs)
        elif np.array_equal(poses[pairs[0][0]][:4], poses[pairs[1][0]][:4]):
            problems.append("the two rotations are one")
        ratios["rank1"] = max(max(planes[k][3], abs(float(np.sqrt(np.sum(planes[k][2] ** 2))) - 1)) for k in present) / E
    else:
        ratios["rank1"] = max(planes[k][3] for k in present) / E
    best = None
    for k in present:
        R, t = planes[k][0], planes[k][1]
        eR = float(np.max(np.abs(R - c["R"])))
        et = float(min(np.max(np.abs(t - c["t"])), np.max(np.abs(t + c["t"])))) / max(c["tau"], 1.0)
        if best is None or max(eR, et) < max(best):
            best = (eR, et)
    ratios["R"], ratios["t"] = best[0] / E, best[1] / E
    for k, v in ratios.items():
        if not v <= 1:
            problems.append("%s: %.3g of the bound" % (k, v))
    return problems, ratios


def solutions_by_index(poses_without_votes):
    """the solutions in the decomposition's own order, read from a run without a single vote: all scores are 0 there, so by the
    order rule position k holds solution 3 - k (one solution: position 0).  Returns the q, t rows."""
    p = np.asarray(poses_without_votes)
    if p[1, 7] == -1:
        assert list(p[:, 7]) == [0, -1, -1, -1], p[:, 7]
        return [p[0, :7].copy()]
    assert list(p[:, 7]) == [0, 0, 0, 0], p[:, 7]
    sols = [p[3 - k, :7].copy() for k in range(4)]
    for a, b in ((0, 1), (2, 3)):   # the twins are neighbours in the solution list
        assert _same_bits(sols[a][:4], sols[b][:4]) and _same_bits(sols[a][4:], -sols[b][4:]), (a, b)
    return sols


def expected_rows(H, sols, r1, r2, flags):
    """what decompose returns for these solutions and rays: (can_decompose, poses 4 x 8, the scores in solution order)"""
    rows = np.full((4, 8), np.nan)
    rows[:, 7] = -1
    rows[:len(sols), :7] = sols
    score = expected_scores(H, rows, r1, r2, flags)
    order = sorted(range(4), key=lambda k: (-score[k], -k))
    out = np.full((4, 8), np.nan)
    for pos, k in enumerate(order):
        out[pos, :7] = rows[k, :7]
        out[pos, 7] = score[k]
    return bool(out[0, 7] > 0), out, score


def check_order(poses):
    """score descending; -1 rows are NaN poses and the others are not"""
    s = [p[7] for p in poses]
    bad = [k for k in range(3) if not s[k] >= s[k + 1]]
    bad += [k for k in range(4) if (s[k] == -1) != bool(np.isnan(poses[k][:7]).all())]
    return bad


class Worst:
    """the worst error-to-bound ratio per quantity and where it came from"""

    def __init__(self):
        self.w = {}

    def add(self, name, r):
        for k, v in r.items():
            if v >= self.w.get(k, (-1.0, ""))[0]:
                self.w[k] = (float(v), name)

    def line(self):
        return json.dumps({k: {"ratio": float("%.3g" % v[0]), "job": v[1]} for k, v in self.w.items()})


# ------------------------------------------------------------------------------------------------------ the conditions
def coverage():
    """the branch and sign counts of the general motions that leave the shortcut (truth, long double)"""
    count = {(i, e): 0 for i in range(3) for e in (1, -1)}
    for c in general():
        f = c["facts"]
        if not f["shortcut"]:
            count[(f["idx"], f["e_sign"])] += 1
    return count


def _self_check():
    cov = coverage()
    for i in range(3):
        assert cov[(i, 1)] + cov[(i, -1)] >= 50, cov
        assert cov[(i, 1)] > 0 and cov[(i, -1)] > 0, cov
    g = general()
    assert sum(c["bounded"] for c in g) >= 0.9 * len(g), sum(c["bounded"] for c in g)
    assert {abs(c["s"]) for c in g} == {10.0 ** k for k in range(-8, 9)} and {c["s"] > 0 for c in g} == {True, False}
    assert min(c["tau"] for c in g) < 2e-3 and max(c["tau"] for c in g) > 2 and all(c["valid"] for c in g)
    bounded_kinds = {c["kind"] for c in drone() if c["bounded"]}
    # A pure climb has S = (2 h + h^2) n n^T of rank one: every 2 x 2 minor of S is zero in truth, so the signs e_ij and the
    # sign of each minor under its square root are decided by rounding - no climb can be bounded by the rule above, whatever
    # R and n; it stays agreement-only and tests/test_decompose_oracle.py reports what the routes return for it.
    assert all(c["facts"]["zero_decides"] for c in drone() if c["kind"] == "climb")
    assert bounded_kinds == set(DRONE_KINDS) - {"climb"}, bounded_kinds
    for c in threshold():
        assert c["valid"] and c["bounded"] != c["improper"], c["name"]


_self_check()

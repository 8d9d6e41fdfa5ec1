"""Systems for the linear algebra of one LM step (relax_lm.hip: lm_build_kernel, chol_tiles_kernel / the launch chain,
back_solve_kernel / back_solve_regions_kernel), and the fp64 / longdouble reference they are checked against.

A case is the input of ochip_debug_lm_step: A = J'J (+ a small diagonal) with J's rows coupling unknowns that the block
envelope (env_end per 64-column block, tail_begin, region_begin: lm_envelope's meaning) allows to be coupled, g, scale,
diagonal and the trust-region radius.  The cases do not depend on the route that factors them: a seam for the resident
chain's factorisation (relax_chain.hip) can take the same list.

The bounds are componentwise (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., thm. 10.3 and 8.5): they
hold whatever the conditioning, and a misplaced or stale tile shows up as O(1) against them."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NB = 64
U = 2.0 ** -53
LD = np.longdouble
C_FACTOR = 4.0    # |W - L L'|_ij <= C (min(i, j) + 2) u sqrt(W_ii W_jj)
C_FORWARD = 4.0   # |L y - gs|_i <= C (i + 2) u (|L| |y| + |gs|)_i
C_BACKWARD = 4.0  # |W x - gs|_i <= C n u (sum_j sqrt(W_ii W_jj) |x_j| + |gs_i|)
C_MODEL = 4.0     # |scal[1] - m| <= C n u * 0.5 sum_i (|x_i gs_i| + D_i x_i^2)
C_FORWARD_ERR = 4.0  # well conditioned only: max |x - x_ref| <= C n u kappa(W) max |x_ref|

SIZES = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193)


# ---- the plan of lm_system_resize, restated --------------------------------------------------------------------------
def plan(n, env_end, tail_begin, region_begin=(), slots=None):
    """Block structure the factorisation stores: stored[I, J] for row block I (0 .. ceil((n + 1) / 64) - 1, the last one
    holds the augmented row n) and column block J; the number of tiles, of tail tiles, the regions and - given the
    device's slots - the claim order (0 column order, 1 tail first, 2 regions)."""
    nbc, nbr = (n + NB - 1) // NB, (n + NB) // NB
    tb = min(tail_begin, n) // NB
    bend, tail_start = [], []
    for J in range(nbc):
        b = max(J + 1, (min(env_end[J], tail_begin) + NB - 1) // NB)
        if J:
            b = max(b, bend[J - 1])  # fill stays inside a monotone envelope
        b = min(b, nbr)
        bend.append(b)
        tail_start.append(max(tb, b, J + 1))
    stored = np.zeros((nbr, max(nbc, 1)), bool)
    for J in range(nbc):
        stored[J:bend[J], J] = True
        stored[tail_start[J]:, J] = True
    limit = min(tb, nbc)
    bounds = []
    rb = list(region_begin)
    if len(rb) > 1 and rb[0] == 0:
        for r in range(len(rb)):
            if not (rb[r] < limit and (r == 0 or rb[r] > rb[r - 1])):
                break
            bounds.append(rb[r])
        bounds.append(limit)
        if len(bounds) < 3:
            bounds = []
    tail_tiles = int(stored[tb:, :nbc].sum()) if nbc else 0
    order = None
    if bounds:
        order = 2
    elif slots is not None:
        order = 1 if tail_tiles * 8 <= slots else 0
    return dict(stored=stored[:, :nbc], n_tiles=int(stored[:, :nbc].sum()), tail_tiles=tail_tiles, tb=tb,
                regions=max(1, len(bounds) - 1), region_bounds=bounds, order=order, bend=bend)


def element_mask(n, stored):
    """(i, j), j <= i < n, inside a stored tile"""
    if n == 0:
        return np.zeros((0, 0), bool)
    blk = np.arange(n) // NB
    return stored[blk[:, None], blk[None, :]] & np.tri(n, dtype=bool)


def allowed_raw(n, env_end, tail_begin, region_of=None):
    """Which couplings (i, j), j < i, the envelope as given (before the plan makes it monotone) admits: i < env_end[j / 64]
    inside the band, every i >= tail_begin; with regions, band unknowns of different regions are not coupled."""
    i = np.arange(n)[:, None]
    j = np.arange(n)[None, :]
    env = np.asarray(env_end, int)[j // NB]
    ok = (j < i) & ((i < np.minimum(env, tail_begin)) | (i >= tail_begin))
    if region_of is not None:
        ok &= (i >= tail_begin) | (region_of[i] == region_of[j])
    return ok


# ---- generators -------------------------------------------------------------------------------------------------------
def jtj(n, allowed, rng, per_row=6, delta=1e-3, weights=None):
    """A = J'J + delta I: J has one row per chosen coupling (i, j) (random values at i and j) and one row per unknown,
    so A's non-zeros are exactly the chosen couplings and the diagonal."""
    A = np.zeros((n, n))
    for i in range(n):
        cols = np.flatnonzero(allowed[i])
        if len(cols) == 0:
            continue
        pick = rng.choice(cols, size=min(per_row, len(cols)), replace=False)
        for j in pick:
            a, b = rng.normal(), rng.normal()
            if weights is not None:
                a, b = a * weights[i], b * weights[j]
            A[i, i] += a * a
            A[j, j] += b * b
            A[i, j] += a * b
            A[j, i] += a * b
    d = rng.uniform(0.5, 1.5, n) * delta
    if weights is not None:
        d = d * weights ** 2
    A[np.diag_indices(n)] += d
    return A


def jacobi(A):
    """scale and diagonal as lm_solve / lm_diag_kernel form them: scale = 1 / (1 + sqrt(diag A)), diagonal =
    clamp(A_ii scale_i^2, 1e-6, 1e32)"""
    d = np.diag(A).copy()
    scale = 1.0 / (1.0 + np.sqrt(d))
    v = d * scale * scale
    return scale, np.minimum(np.maximum(v, 1e-6), 1e32)


class Case:
    def __init__(self, name, A, g, scale, diagonal, radius, env_end, tail_begin, region_begin=(), expect="ok", well=False):
        self.name, self.A, self.g, self.scale, self.diagonal, self.radius = name, A, g, scale, diagonal, radius
        self.env_end, self.tail_begin, self.region_begin = list(env_end), int(tail_begin), list(region_begin)
        self.expect, self.well = expect, well  # expect: "ok", "fail" (not PD) or "nan_g"; well: kappa(W) < 1e4
        self.n = len(g)

    def __repr__(self):
        return self.name

    @functools.cached_property
    def plan(self):
        return plan(self.n, self.env_end, self.tail_begin, self.region_begin)

    @functools.cached_property
    def mask(self):
        return element_mask(self.n, self.plan["stored"])

    @functools.cached_property
    def ref(self):
        return reference(self)


def _make(name, n, env_end, tail_begin, seed, region_begin=(), region_of=None, per_row=6, delta=1e-3, radius=1e2,
          expect="ok", well=False, weights=None, check=True):
    rng = np.random.default_rng(seed)
    allowed = allowed_raw(n, env_end, tail_begin, region_of)
    A = jtj(n, allowed, rng, per_row=per_row, delta=delta, weights=weights)
    scale, diagonal = jacobi(A)
    g = rng.normal(size=n) * np.sqrt(np.diag(A))
    c = Case(name, A, g, scale, diagonal, radius, env_end, tail_begin, region_begin, expect=expect, well=well)
    if check:
        check_inside(c)
    return c


def check_inside(c):
    """A's couplings and the exact factor lie inside the stored tiles (the generator's own assertion; A was drawn inside
    the envelope as given, the factor's fill must stay inside the envelope as the plan makes it monotone; exact zeros:
    LAPACK's factor of a profile matrix has no fill outside the profile)."""
    n = c.n
    if n == 0:
        return
    low = np.tril(c.A, -1) != 0
    assert not (low & ~c.mask).any(), f"{c.name}: A outside the stored tiles"
    if c.expect == "ok":
        W = full(reference_W(c))
        L = np.linalg.cholesky(W)
        assert not ((L != 0) & ~c.mask).any(), f"{c.name}: exact factor outside the envelope"


def band_env(n, half):
    """env_end of a block band reaching `half` unknowns below each column block"""
    return [min((J + 1) * NB + half, n) for J in range((n + NB - 1) // NB)]


def _regions_of(n, starts_blocks, tail_begin):
    r = np.zeros(n, int)
    for k, b in enumerate(starts_blocks):
        r[b * NB:] = k
    r[tail_begin:] = -1
    return r


def basic_cases():
    cases = []
    for n in SIZES:
        nbc = (n + NB - 1) // NB
        cases.append(_make(f"dense_tail_n{n}", n, [n] * nbc, 0, 100 + n, per_row=8, well=True))
        cases.append(_make(f"dense_band_n{n}", n, [n] * nbc, n, 200 + n, per_row=8, well=True))
    for n in (127, 128, 129, 191, 192, 193):
        cases.append(_make(f"band_n{n}", n, band_env(n, 24), n, 300 + n, well=True))
    for n, t in ((193, 1), (192, 3), (191, 64), (193, 65), (129, 3)):
        tb = n - t
        cases.append(_make(f"band_tail{t}_n{n}", n, band_env(n, 24), tb, 400 + n + t, well=True))
    cases.append(_make("band_tail_mid_block_n193", 193, band_env(193, 40), 81, 501, well=True))   # 64 + 17
    cases.append(_make("band_tail_mid_block_n191", 191, band_env(191, 10), 145, 502, well=True))  # 128 + 17
    cases.append(_make("tail_begin_eq_n_n192", 192, band_env(192, 64), 192, 503, well=True))
    # non-monotone env_end: block 0 reaches further down than block 1 claims; the plan makes it monotone
    cases.append(_make("nonmonotone_n193", 193, [192, 100, 150, 193], 193, 504, well=True))
    cases.append(_make("nonmonotone_tail_n256", 256, [250, 90, 200, 256], 230, 505, well=True))
    # regions: 2 regions; 3 regions with a single-block one and a last region inside the tail's first block (folded)
    n, tb = 330, 266
    rb = [0, 2]
    env = [128, 128, 256, 256, 330, 330][:(n + 63) // 64]
    cases.append(_make("regions2_n330", n, env, tb, 506, region_begin=rb, region_of=_regions_of(n, rb, tb), well=True))
    n, tb = 468, 394
    rb = [0, 2, 3, 6]
    env = [128, 128, 192, 384, 384, 384, 468, 468]
    cases.append(_make("regions3_folded_n468", n, env, tb, 507, region_begin=rb, region_of=_regions_of(n, rb, tb), well=True))
    return cases


def conditioning_cases():
    cases = []
    n, tb = 193, 190
    env = band_env(n, 30)
    # graded: the damping diagonal spans the clamp range 1e-6 .. 1e32 of lm_diag_kernel, the system graded alike
    rng = np.random.default_rng(601)
    spread = np.geomspace(1e-6, 1e32, n)[rng.permutation(n)]
    c = _make("graded_n193", n, env, tb, 602, weights=np.sqrt(spread), check=False)
    c.scale = np.ones(n)
    c.diagonal = spread
    c.radius = 1e3
    check_inside(c)
    cases.append(c)
    # kappa(W) ~ 1e8 / 1e12: a chain of differences (a graph Laplacian: singular, the constant vector its null space)
    # damped by diagonal / radius
    for target, radius in ((1e8, 1e8), (1e12, 1e12)):
        rng = np.random.default_rng(int(np.log10(target)))
        A = np.zeros((n, n))
        for i in range(1, n):
            for j in rng.choice(np.flatnonzero(allowed_raw(n, env, tb)[i]), size=min(3, i), replace=False):
                w = rng.uniform(0.5, 2.0)
                A[i, i] += w
                A[j, j] += w
                A[i, j] -= w
                A[j, i] -= w
        scale, diagonal = jacobi(A)
        g = rng.normal(size=n)
        c = Case(f"kappa{int(np.log10(target))}_n193", A, g, scale, diagonal, radius, env, tb)
        check_inside(c)
        cases.append(c)
    # a nearly singular 12-unknown point-like block (singular values of J down to 3e-7: kappa(A) ~ 1e13) with radius 1e16,
    # so that the damping adds nothing
    rng = np.random.default_rng(603)
    q1, _ = np.linalg.qr(rng.normal(size=(30, 12)))
    q2, _ = np.linalg.qr(rng.normal(size=(12, 12)))
    Jm = (q1 * np.geomspace(1.0, 3e-7, 12)) @ q2.T
    A = Jm.T @ Jm
    scale, diagonal = jacobi(A)
    c = Case("near_singular_point_n12", A, rng.normal(size=12) * 10, scale, diagonal, 1e16, [12], 0)
    check_inside(c)
    cases.append(c)
    return cases


def failure_cases():
    """Non-positive pivots placed in block 0, a middle band block, the tail and the last partial block; an exactly singular
    PSD A with tiny damping (must NOT fail); NaN in A; NaN in g."""
    cases = []

    def negative_pivot(name, n, env, tb, p, seed):
        c = _make(name, n, env, tb, seed, expect="fail", check=False)
        # pivot p of the exact factor becomes -1 (up to the damping): W_pp minus what the rows above take out of it
        W = full(reference_W(c))
        L = np.linalg.cholesky(W)
        piv = L[p, p] ** 2
        c.A[p, p] -= (piv + 1.0) / (c.scale[p] ** 2)
        check_inside(c)
        return c

    n, tb = 193, 190
    env = band_env(n, 30)
    cases.append(negative_pivot("notpd_block0_n193", n, env, tb, 5, 701))
    cases.append(negative_pivot("notpd_band_n193", n, env, tb, 100, 702))
    cases.append(negative_pivot("notpd_tail_n193", n, env, tb, 191, 703))
    cases.append(negative_pivot("notpd_last_partial_n150", 150, band_env(150, 30), 150, 140, 704))
    # exactly singular PSD A (J'J of a rank-deficient J: unknowns 0 .. 9 never appear) with tiny damping: W is PD
    n = 129
    rng = np.random.default_rng(705)
    env = band_env(n, 24)
    allowed = allowed_raw(n, env, n)
    allowed[:10, :] = False
    allowed[:, :10] = False
    A = jtj(n, allowed, rng, delta=0.0)
    scale, diagonal = jacobi(A)
    c = Case("singular_psd_damped_n129", A, rng.normal(size=n), scale, diagonal, 1e4, env, n)
    check_inside(c)
    cases.append(c)
    c = _make("nan_in_A_n65", 65, [65, 65], 0, 706, expect="fail", check=False)
    c.A[40, 3] = c.A[3, 40] = np.nan
    cases.append(c)
    c = _make("nan_in_g_n65", 65, [65, 65], 0, 707, expect="nan_g")
    c.g[30] = np.nan
    cases.append(c)
    return cases


@functools.lru_cache(maxsize=None)
def big_case():
    """n = 3003: the 1 000-camera system (3 unknowns per camera in a band, 3 plane unknowns as the dense tail), in two
    regions"""
    n, tb = 3003, 3000
    rb = [0, 24]
    region_of = _regions_of(n, rb, tb)
    env = []
    for J in range((n + NB - 1) // NB):
        end = min((J + 1) * NB + 100, tb)
        env.append(min(end, 24 * NB) if J < 24 else end)  # region 0's columns reach no row of region 1
    return _make("cameras1000_n3003", n, env, tb, 801, region_begin=rb, region_of=region_of, per_row=4, well=True)


@functools.lru_cache(maxsize=None)
def column_order_case(slots):
    """A fully dense system (every block a tail block) whose tail tiles exceed an eighth of the device's slots: the
    plan's plain column order"""
    nbr = 1
    while nbr * (nbr + 1) // 2 * 8 <= slots:
        nbr += 1
    n = nbr * NB - 1  # (the augmented row in the last block: nbr row blocks, nbr column blocks)
    return _make(f"column_order_n{n}", n, [n] * ((n + NB - 1) // NB), 0, 900, per_row=6, well=True)


# ---- systems of an actual relax problem (their J'J comes from the device: ochip_relaxg_evaluate) -----------------------
REAL_SCENES = ((8, 8, 2), (12, 16, 3))  # camera rows, columns, mesh vertices per side


def mesh_scene(rows, cols, seed=0, mesh=3, spacing=4.0, height=10.0):
    """A camera grid over a mesh x mesh vertex ground mesh, as the general engine takes it: the cameras look down (slightly
    perturbed), every pair of neighbouring cameras shares 2-ray blocks over the triangles of their common ground, every
    camera has its PointsDownwardsPrior, every mesh edge its DifferenceCost and every vertex its anchor.  A mesh of at
    most 8 vertices is the engine's dense tail; larger ones join the cameras in the band."""
    rng = np.random.default_rng(seed)
    cam = np.array([[c * spacing, r * spacing, height] for r in range(rows) for c in range(cols)], float)
    n_cams = len(cam)
    q = np.zeros((n_cams, 4))
    for i in range(n_cams):  # DOWN (pi about x) times a small rotation
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        a = 0.02
        v, w = ax * np.sin(a / 2), np.cos(a / 2)
        q[i] = [w, -v[2], v[1], -v[0]]  # (1, 0, 0, 0) * (v, w), xyzw
        q[i] /= np.linalg.norm(q[i])
    x0, x1 = -spacing, cols * spacing
    y0, y1 = -spacing, rows * spacing
    vx, vy = np.meshgrid(np.linspace(x0, x1, mesh), np.linspace(y0, y1, mesh))
    vert_xy = np.stack([vx.ravel(), vy.ravel()], 1)
    n_verts = mesh * mesh
    vert_z = rng.normal(size=n_verts) * 0.1
    tris = []
    for r in range(mesh - 1):
        for c in range(mesh - 1):
            a, b, d, e = mesh * r + c, mesh * r + c + 1, mesh * (r + 1) + c, mesh * (r + 1) + c + 1
            tris += [(a, b, e), (a, e, d)]
    tris = np.array(tris)

    def tri_of(p):
        for k, t in enumerate(tris):
            P = vert_xy[t]
            m = np.array([P[1] - P[0], P[2] - P[0]]).T
            l1, l2 = np.linalg.solve(m, p - P[0])
            if l1 >= -1e-12 and l2 >= -1e-12 and l1 + l2 <= 1 + 1e-12:
                return k
        raise AssertionError(p)

    blk_n, blk_ray_off, blk_tri, ray_cam, ray_dir = [], [0], [], [], []
    for a in range(n_cams):
        for b in range(a + 1, n_cams):
            if np.max(np.abs(cam[a, :2] - cam[b, :2])) > spacing * 1.01:
                continue
            for _ in range(3):
                p = 0.5 * (cam[a, :2] + cam[b, :2]) + rng.uniform(-1, 1, 2)
                k = tri_of(p)
                z = float(np.mean(vert_z[tris[k]]))
                blk_n.append(2)
                blk_tri.append(tris[k])
                for c_ in (a, b):
                    d = np.array([p[0], p[1], z]) - cam[c_]
                    d /= np.linalg.norm(d)
                    ray_cam.append(c_)
                    ray_dir.append([d[0], -d[1], -d[2]])  # world -> camera frame of DOWN
                blk_ray_off.append(blk_ray_off[-1] + 2)
    diff = [(mesh * r + c, mesh * r + c + 1) for r in range(mesh) for c in range(mesh - 1)] + \
           [(mesh * r + c, mesh * (r + 1) + c) for r in range(mesh - 1) for c in range(mesh)]
    return dict(cam_pos=cam, cam_q=q, cam_optimize=np.ones(n_cams, np.uint8), vert_xy=vert_xy, vert_z=vert_z,
                vert_optimize=np.ones(n_verts, np.uint8), blk_n=np.array(blk_n, np.uint8), blk_ray_off=np.array(blk_ray_off),
                blk_tri=np.array(blk_tri).ravel(), ray_cam=np.array(ray_cam), ray_dir=np.array(ray_dir).ravel(),
                down_cam=np.arange(n_cams), down_weight=1e-3, diff_v=np.array(diff).ravel(), diff_weight=1e-4,
                anchor_weight=1e-5, huber_a=np.pi / 180, model=[600.0, 400, 300, 0, 0, 0, 0, 0])


def real_case(name, JtJ, Jtr, order, n_cams, n_verts, radius=1e4):
    """The step system of an evaluated relax problem: scale and diagonal as lm_solve forms them from its first Jacobian,
    Ceres' initial trust region, and the envelope derived from J'J's non-zero pattern (vertex heights behind every camera
    are the dense tail; per column block the last band row it reaches)."""
    n = len(Jtr)
    cam_t = order[:n_cams]
    vert_t = order[n_cams:n_cams + n_verts]
    assert (cam_t >= 0).all() and (vert_t >= 0).all()
    tail_begin = int(vert_t.min()) if vert_t.min() > cam_t.max() else n
    env_end = []
    for J in range((n + NB - 1) // NB):
        cols = np.tril(JtJ[:tail_begin, J * NB:(J + 1) * NB] != 0)
        rows = np.flatnonzero(cols.any(axis=1))
        env_end.append(max(min((J + 1) * NB, tail_begin), int(rows.max()) + 1 if len(rows) else 0))
    scale, diagonal = jacobi(JtJ)
    c = Case(name, JtJ, Jtr, scale, diagonal, radius, env_end, tail_begin, well=True)
    check_inside(c)
    return c


def golden_real_cases():
    """the systems of REAL_SCENES as the engine evaluated them when they were recorded (tests/golden/lm_mesh_*.npz:
    J'J's lower triangle, J'r, the unknowns' order); test_gpu_lm_linear.py also evaluates the scenes afresh"""
    cases = []
    for rows, cols, mesh in REAL_SCENES:
        d = np.load(os.path.join(GOLDEN, f"lm_mesh_{rows}x{cols}_{mesh}.npz"))
        n = int(d["n"])
        A = np.zeros((n, n))
        A[d["i"], d["j"]] = d["v"]
        A[d["j"], d["i"]] = d["v"]
        cases.append(real_case(f"golden_mesh_{rows}x{cols}_{mesh}", A, d["Jtr"], d["order"], rows * cols, mesh * mesh))
    return cases


@functools.lru_cache(maxsize=None)
def all_cases():
    return basic_cases() + conditioning_cases() + failure_cases() + golden_real_cases()


# ---- the reference ----------------------------------------------------------------------------------------------------
def reference_W(c):
    """W = S A S + D as lm_build_kernel forms it, lower triangle, (n + 1) x n: row n = gs = S g.  W_ij = (a s_i) s_j,
    W_ii += dd * dd with dd = sqrt(diagonal_i / radius)."""
    n = c.n
    W = np.zeros((n + 1, n))
    if n == 0:
        return W
    low = np.tril((c.A * c.scale[:, None]) * c.scale[None, :])
    dd = np.sqrt(c.diagonal / c.radius)
    lm = dd * dd
    low[np.diag_indices(n)] += lm
    W[:n] = low
    W[n] = c.g * c.scale
    return W


def lm_diag(c):
    dd = np.sqrt(c.diagonal / c.radius)
    return dd * dd


def full(Wa):
    """the symmetric n x n matrix of an (n + 1) x n lower triangle with the augmented row"""
    n = Wa.shape[1]
    low = np.tril(Wa[:n])
    return low + np.tril(low, -1).T


def reference(c):
    """fp64 LAPACK factor and solves (None where the system is not PD)"""
    import scipy.linalg as sl

    Wa = reference_W(c)
    W = full(Wa)
    gs = Wa[c.n]
    try:
        L = np.linalg.cholesky(W)
    except np.linalg.LinAlgError:
        L = None
    if L is None or not np.all(np.isfinite(L)) or not np.all(np.isfinite(gs)):
        return dict(W=Wa, L=None, y=None, x=None)
    y = sl.solve_triangular(L, gs, lower=True)
    x = sl.cho_solve((L, True), gs)
    return dict(W=Wa, L=L, y=y, x=x)


def factor_residual(Wa, L, stored):
    """|W - L L'| on the lower triangle, longdouble, tile by tile over the stored tiles (L must vanish outside them)"""
    n = L.shape[0]
    R = np.zeros((n, n))
    nbc = (n + NB - 1) // NB
    Ll = L.astype(LD)
    sl_ = [slice(k * NB, min((k + 1) * NB, n)) for k in range(nbc)]
    for J in range(nbc):
        for I in range(J, nbc):
            if not stored[I, J]:
                continue
            acc = Wa[sl_[I], sl_[J]].astype(LD)
            for K in range(J + 1):
                if stored[I, K] and stored[J, K]:
                    acc = acc - Ll[sl_[I], sl_[K]] @ Ll[sl_[J], sl_[K]].T
            R[sl_[I], sl_[J]] = np.abs(acc).astype(np.float64)
    return np.tril(R)


def factor_ratio(Wa, L, stored):
    """max over the lower triangle of |W - L L'|_ij / (C (min(i, j) + 2) u sqrt(W_ii W_jj))"""
    n = L.shape[0]
    R = factor_residual(Wa, L, stored)
    d = np.sqrt(np.abs(np.diag(Wa[:n])))
    i = np.arange(n)
    bound = C_FACTOR * (np.minimum(i[:, None], i[None, :]) + 2) * U * (d[:, None] * d[None, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(np.tri(n, dtype=bool), R / bound, 0.0)
    return float(np.max(r)) if n else 0.0


def forward_ratio(L, y, gs):
    """max_i |L y - gs|_i / (C (i + 2) u (|L| |y| + |gs|)_i), longdouble residual"""
    n = len(y)
    if n == 0:
        return 0.0
    r = np.abs(L.astype(LD) @ y.astype(LD) - gs.astype(LD)).astype(np.float64)
    b = C_FORWARD * (np.arange(n) + 2) * U * (np.abs(L) @ np.abs(y) + np.abs(gs))
    return float(np.max(r / b))


def backward_ratio(Wa, x):
    """max_i |W x - gs|_i / (C n u (sum_j sqrt(W_ii W_jj) |x_j| + |gs_i|)), longdouble residual"""
    n = len(x)
    if n == 0:
        return 0.0
    W = full(Wa)
    gs = Wa[n]
    r = np.abs(W.astype(LD) @ x.astype(LD) - gs.astype(LD)).astype(np.float64)
    d = np.sqrt(np.abs(np.diag(W)))
    b = C_BACKWARD * n * U * (d * np.dot(d, np.abs(x)) + np.abs(gs))
    return float(np.max(r / b))


def model_change(c, x):
    """0.5 sum(x_i gs_i + D_i x_i^2) in longdouble, and the scale of its rounding (0.5 sum |x_i gs_i| + D_i x_i^2)"""
    gs = (c.g * c.scale).astype(LD)
    D = lm_diag(c).astype(LD)
    xl = x.astype(LD)
    m = LD(0.5) * np.sum(xl * gs + D * xl * xl)
    s = LD(0.5) * np.sum(np.abs(xl * gs) + D * xl * xl)
    return float(m), float(s)


def model_ratio(c, x, scal1):
    m, s = model_change(c, x)
    if c.n == 0:
        return 0.0 if scal1 == 0.0 else np.inf
    return abs(scal1 - m) / (C_MODEL * c.n * U * s)


def kappa(Wa):
    ev = np.linalg.eigvalsh(full(Wa))
    return float(ev[-1] / ev[0])


def forward_error_ratio(Wa, x, x_ref, kap=None):
    """well conditioned only: max |x - x_ref| / (C n u kappa max |x_ref|)"""
    n = len(x)
    kap = kappa(Wa) if kap is None else kap
    return float(np.max(np.abs(x - x_ref)) / (C_FORWARD_ERR * n * U * kap * np.max(np.abs(x_ref))))

"""Seeded inputs of homography_model::fitInliers / fit / evaluate (src/model_inliers/homography_model.cpp:19-118) at the
edges the pipeline tests never reach, a numpy restatement of the operation in any precision, and the bounds the fp64
results (the oracle's and the device's) are held to against the 80-bit long-double restatement.  Data and arithmetic only;
no device.

A job is the input of one fitInliers + evaluate: the pixels of both images, a distortion-free camera model per image (so
that every route starts from the same doubles: rays_of() below is image_to_3d without distortion, and
tests/test_homography_fit_oracle.py holds it bit-equal to the oracle's), the inlier flags and a name.  The *input of the
operation* is the fp64 unit rays; the reference divides them by z in long double and goes on from there.

The reference is "solve these nine equations in this order": the pivot sequence and the rank are decided in fp64 (checked
bit for bit against the oracle) and forced on the long-double elimination.  Where the long double's own choice would have
differed is recorded (`own_differs`) and reported, not used."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, (
    "numpy.longdouble is not the 80-bit extended type here (eps %g): the long-double homography reference needs a 64-bit "
    "significand; restate it in C++ long double under oracle/ as oracle/relax_eval.cpp does" % np.finfo(LD).eps)

U = 2.0 ** -53
U_LD = 2.0 ** -64
EPS64 = 2.0 ** -52           # Eigen's NumTraits<double>::epsilon() in FullPivLU::rank()
THR = 0.005                  # homography_model::inlier_threshold
C_FIT = 2.0 ** 8             # the one constant of every bound (calibration: tests/test_homography_fit_oracle.py)
# H^-1, the errors and the score of a job are held to their bounds only while C_FIT u kappa kappa(H) stays below this: past
# it the inverse of the reference itself has no correct digit left to compare with (singular H of a rank-deficient fit)
INVERTIBLE = 2.0 ** -10

MODEL = np.array([3000.0, 2000.0, 1500.0, 0, 0, 0, 0, 0])   # a 4000 x 3000 image, no distortion
UNIT = np.array([1.0, 0.0, 0.0, 0, 0, 0, 0, 0])             # pixels are the normalised coordinates themselves
WELL_POSED = ("scenes", "few", "placement", "ties", "deficient")


# ---------------------------------------------------------------------------------------------------------- rays
def rays_of(px, model):
    """image_to_3d of a model without distortion: (px - pp) / f, homogeneous().normalized() (divide by the norm if the
    squared norm is positive - an overflowed norm gives the ray 0, 0, 0, a NaN leaves the vector as it is)"""
    px = np.asarray(px, np.float64).reshape(-1, 2)
    with np.errstate(all="ignore"):
        ux, uy = (px[:, 0] - model[1]) / model[0], (px[:, 1] - model[2]) / model[0]
        z = ux * ux + uy * uy + 1.0
        n = np.sqrt(z)
        pos = z > 0
        one = np.ones_like(ux)
        return np.stack([np.where(pos, ux / n, ux), np.where(pos, uy / n, uy), np.where(pos, one / n, one)], 1)


def job_rays(job):
    return rays_of(job["px1"], job["model1"]), rays_of(job["px2"], job["model2"])


def coords(r1, r2, dtype):
    """x, y, x', y' = the rays divided by z, in dtype"""
    r1, r2 = np.asarray(r1, dtype), np.asarray(r2, dtype)
    with np.errstate(all="ignore"):
        return r1[:, 0] / r1[:, 2], r1[:, 1] / r1[:, 2], r2[:, 0] / r2[:, 2], r2[:, 1] / r2[:, 2]


# ------------------------------------------------------------------------------------------------- the operation
def dlt_system(x, y, x_, y_, flip=False):
    """the (2 n + 1) x 9 system of homography_model.cpp:26-35,61-70 (two rows per correspondence, then 0 .. 0 1)"""
    n = len(x)
    A = np.zeros((2 * n + 1, 9), x.dtype)
    with np.errstate(all="ignore"):
        A[0:2 * n:2, 0], A[0:2 * n:2, 1], A[0:2 * n:2, 2] = -x, -y, -1
        A[0:2 * n:2, 6], A[0:2 * n:2, 7], A[0:2 * n:2, 8] = x * x_, y * x_, x_
        A[1:2 * n:2, 3], A[1:2 * n:2, 4], A[1:2 * n:2, 5] = -x, -y, -1
        A[1:2 * n:2, 6], A[1:2 * n:2, 7], A[1:2 * n:2, 8] = x * y_, y * y_, y_
    if flip:                         # (mutant) one sign of the DLT rows wrong
        A[1:2 * n:2, 7] = -A[1:2 * n:2, 7]
    A[2 * n, 8] = 1
    return A


def _search(A, k, last=False, second=False):
    """Eigen's pivot search over the corner A[k:, k:]: column by column, strict '>', so the first maximum of that order; a
    NaN in the first cell sticks, a NaN anywhere else never wins.  (mutants) last: '>=' - the last maximum; second: the
    next-best candidate"""
    sub = np.abs(A[k:, k:])
    if np.isnan(sub[0, 0]):
        return k, k, sub[0, 0]
    flat = np.where(np.isnan(sub), -1.0, sub).T.ravel()
    if second:
        idx = int(np.argsort(-flat, kind="stable")[1])
    elif last:
        idx = len(flat) - 1 - int(np.argmax(flat[::-1]))
    else:
        idx = int(np.argmax(flat))
    nr = sub.shape[0]
    return k + idx % nr, k + idx // nr, flat[idx]


def full_piv_lu_solve(A, forced=None, tie_last=False, swap_step=None, truncate=True):
    """FullPivLU<Matrix<T, rows, 9>>(A).solve(e_last) in A's dtype: computeInPlace, rank() with the fp64 epsilon,
    _solve_impl.  forced = the `lu` dict of another run: its transpositions, stop and rank are taken as given.
    Returns (solution[9], lu) with lu = dict(rowT, colT, nonzero, rank, diag, pivot_rows, own_differs)."""
    A = A.copy()
    T = A.dtype.type
    rows, cols = A.shape
    size = min(rows, cols)
    rowT, colT = list(range(size)), list(range(size))
    origin = np.arange(rows)             # which row of the system sits where
    nonzero, maxpivot, own_differs = size, T(0), 0
    with np.errstate(all="ignore"):
        for k in range(size):
            br, bc, biggest = _search(A, k, last=tie_last, second=(swap_step == k))
            if forced is not None:
                if k >= forced["nonzero"]:
                    nonzero = k
                    break
                own_differs += int((br, bc) != (forced["rowT"][k], forced["colT"][k]))
                br, bc = forced["rowT"][k], forced["colT"][k]
                biggest = np.abs(A[br, bc])
            elif biggest == 0:
                nonzero = k
                break
            if biggest > maxpivot:
                maxpivot = biggest
            rowT[k], colT[k] = br, bc
            if br != k:
                A[[k, br]] = A[[br, k]]
                origin[[k, br]] = origin[[br, k]]
            if bc != k:
                A[:, [k, bc]] = A[:, [bc, k]]
            A[k + 1:, k] = A[k + 1:, k] / A[k, k]
            if k < size - 1:
                A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - np.outer(A[k + 1:, k], A[k, k + 1:])
        diag = np.array([A[i, i] for i in range(size)])
        premult = np.abs(maxpivot) * T(EPS64 * size)
        if forced is not None:
            rank = forced["rank"]
        elif truncate:
            rank = int(np.sum(np.abs(diag[:nonzero]) > premult))
        else:                            # (mutant) every non-zero pivot used
            rank = int(np.sum(np.abs(diag[:nonzero]) > 0))
        sol = np.zeros(9, A.dtype)
        lu = dict(rowT=rowT, colT=colT, nonzero=nonzero, rank=rank, diag=diag, pivot_rows=origin[:size].copy(),
                  own_differs=own_differs)
        if rank == 0:
            return sol, lu
        c = np.zeros(rows, A.dtype)
        c[rows - 1] = 1
        for k in range(size):
            c[[k, rowT[k]]] = c[[rowT[k], k]]
        for j in range(size):
            c[j + 1:size] = c[j + 1:size] - c[j] * A[j + 1:size, j]
        for j in range(rank - 1, -1, -1):
            c[j] = c[j] / A[j, j]
            c[:j] = c[:j] - c[j] * A[:j, j]
        perm = list(range(9))
        for k in range(size):
            perm[k], perm[colT[k]] = perm[colT[k]], perm[k]
        for i in range(rank):
            sol[perm[i]] = c[i]
    return sol, lu


def _cof(m, i, j):
    i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
    return m[i1, j1] * m[i2, j2] - m[i1, j2] * m[i2, j1]


def inverse3(m):
    """Eigen's compute_inverse of a 3 x 3: cofactors of column 0 for the determinant, cofactor(j, i) * (1 / det)"""
    with np.errstate(all="ignore"):
        d = _cof(m, 0, 0) * m[0, 0] + _cof(m, 1, 0) * m[1, 0] + _cof(m, 2, 0) * m[2, 0]
        inv = m.dtype.type(1) / d
        return np.array([[_cof(m, c, r) * inv for c in range(3)] for r in range(3)], m.dtype)


def kappa_of(lu):
    d = np.abs(np.asarray(lu["diag"][:lu["rank"]], LD))
    if len(d) == 0 or not np.all(np.isfinite(d)) or d.min() == 0:
        return np.inf
    return float(d.max() / d.min())


def solve_coords(x, y, x_, y_, forced=None, normalise=True, flip=False, **mut):
    """fitInliers on the correspondences given by their coordinates (all of them inliers), in their dtype"""
    A = dlt_system(x, y, x_, y_, flip=flip)
    sol, lu = full_piv_lu_solve(A, forced=forced, **mut)
    with np.errstate(all="ignore"):
        H = sol.reshape(3, 3) / sol[8] if normalise else sol.reshape(3, 3).copy()
    return dict(H=H, Hinv=inverse3(H), sol=sol, lu=lu, rank=lu["rank"], kappa=kappa_of(lu), system=A)


def replay(r1, r2, flags, dtype=np.float64, forced=None, **kw):
    """homography_model::fitInliers on the flagged correspondences of the unit rays r1, r2, in dtype"""
    f = np.asarray(flags, bool)
    x, y, x_, y_ = coords(r1[f], r2[f], dtype)
    return solve_coords(x, y, x_, y_, forced=forced, **kw)


def reference(r1, r2, flags, **kw):
    """the same elimination in long double with the pivot sequence, the stop and the rank of the fp64 replay"""
    d = replay(r1, r2, flags, np.float64)
    ref = replay(r1, r2, flags, LD, forced=d["lu"], **kw)
    ref["fp64"] = d
    return ref


def replay_sample(xy16, dtype=np.float64, forced=None):
    """homography_model::fit of one minimal sample: four correspondences x (x, y, x', y'), already divided by z"""
    c = np.asarray(xy16, np.float64).reshape(4, 4).astype(dtype)
    return solve_coords(c[:, 0], c[:, 1], c[:, 2], c[:, 3], forced=forced)


def reference_sample(xy16):
    d = replay_sample(xy16)
    ref = replay_sample(xy16, LD, forced=d["lu"])
    ref["fp64"] = d
    return ref


def degenerate(xy16):
    """checkSampleDegeneracy (homography_model.cpp:120-136): any three of the four image-1 points within 1e-10 of a line"""
    p = np.asarray(xy16, np.float64).reshape(4, 4)[:, :2]
    with np.errstate(all="ignore"):
        for i in range(4):
            for j in range(i + 1, 4):
                for k in range(j + 1, 4):
                    v1, v2 = p[j] - p[i], p[k] - p[i]
                    if abs(v1[0] * v2[1] - v1[1] * v2[0]) < 1e-10:
                        return True
    return False


def evaluate_ld(H, Hinv, r1, r2, thr=THR):
    """homography_model::error / evaluate (homography_model.cpp:89-118) in long double: errors, flags, MSAC terms"""
    H, Hinv = np.asarray(H, LD), np.asarray(Hinv, LD)
    x, y, x_, y_ = coords(r1, r2, LD)
    with np.errstate(all="ignore"):
        f = H @ np.stack([x, y, np.ones_like(x)]) if len(x) else np.zeros((3, 0), LD)
        b = Hinv @ np.stack([x_, y_, np.ones_like(x)]) if len(x) else np.zeros((3, 0), LD)
        fx, fy = f[0] / f[2] - x_, f[1] / f[2] - y_
        bx, by = b[0] / b[2] - x, b[1] / b[2] - y
        e = np.sqrt(((fx * fx + fy * fy) + (bx * bx + by * by)) / LD(2))
        inl = e < LD(thr)
        term = np.where(inl, LD(1) - (e / LD(thr)) ** 2, LD(0))
    return dict(err=e, flags=inl.astype(np.uint8), term=term)


# ------------------------------------------------------------------------------------------------------ bounds
def kappa_H(H):
    """the 2-norm condition number of the long-double H (inf where it is singular or not finite)"""
    H = np.asarray(H, np.float64)
    return float(np.linalg.cond(H)) if np.all(np.isfinite(H)) else np.inf


def _absmax(a):
    return float(np.max(np.abs(a))) if np.size(a) else 0.0


def bounds(ref, r1, r2):
    """ref = reference(...) of a bounded job.  H: C u kappa |H_ld|max.  H^-1: the same with kappa(H) multiplied in.  Per
    correspondence the error may be off by C u kappa (e_i + |x_i|max), which decides whether its flag is decidable; the
    score (MSAC sum / M) by C u kappa (1 + n_in) / M over the decidable correspondences, n_in = the reference's inliers."""
    k = ref["kappa"]
    ev = evaluate_ld(ref["H"], ref["Hinv"], r1, r2)
    M = len(r1)
    with np.errstate(all="ignore"):
        kH = kappa_H(ref["H"])
        invertible = bool(np.all(np.isfinite(np.asarray(ref["Hinv"], np.float64))) and C_FIT * U * k * kH < INVERTIBLE)
        x, y, x_, y_ = coords(r1, r2, LD)
        xmax = np.max(np.abs(np.stack([x, y, x_, y_, np.ones_like(x)])), axis=0) if M else np.zeros(0, LD)
        slack = C_FIT * U * k * (ev["err"] + xmax)
        undecidable = ~(np.abs(ev["err"] - LD(THR)) > slack) & np.isfinite(ev["err"])
    n_in = int(np.sum(ev["flags"][~undecidable]))
    return dict(H=C_FIT * U * k * _absmax(ref["H"]), Hinv=C_FIT * U * k * kH * _absmax(ref["Hinv"]) if invertible else None,
                score=C_FIT * U * k * (1 + n_in) / max(M, 1), invertible=invertible, undecidable=undecidable, eval=ev, n_in=n_in)


def ratios(H, Hinv, score, flags, ref, b, err=None):
    """error-to-bound ratios of an fp64 result (score = MSAC sum / M; Hinv may be None), and the number of flags that
    differ from the long-double flags outside the undecidable set.  Where a job has undecidable correspondences the score
    is summed again from the fp64 errors `err` without them."""
    with np.errstate(all="ignore"):
        r = dict(H=_absmax(np.asarray(H, LD) - ref["H"]) / b["H"])
        if b["invertible"]:
            if Hinv is not None:
                r["Hinv"] = _absmax(np.asarray(Hinv, LD) - ref["Hinv"]) / b["Hinv"]
            keep = ~b["undecidable"]
            M = len(keep)
            s_ld = float(np.sum(b["eval"]["term"][keep])) / max(M, 1)
            r["score_ld"] = s_ld
            if np.any(b["undecidable"]):
                score = None if err is None else score_without(err, b["undecidable"], M)
            if score is not None:
                r["score"] = abs(score - s_ld) / b["score"]
            r["flags_off"] = int(np.sum((np.asarray(flags, np.uint8) != b["eval"]["flags"]) & keep))
    return r


def score_without(err, undecidable, M, thr=THR):
    """the MSAC sum / M of fp64 errors, the undecidable correspondences left out (for jobs that have some)"""
    e = np.asarray(err, np.float64)
    with np.errstate(all="ignore"):
        t = np.where((e < thr) & ~undecidable, 1.0 - (e / thr) * (e / thr), 0.0)
    return float(np.sum(t.astype(LD))) / max(M, 1)


# ------------------------------------------------------------------------------------------------------- scenes
def _rot(w, dtype=np.float64):
    w = np.asarray(w, dtype)
    th = np.sqrt(w @ w)
    if th == 0:
        return np.eye(3, dtype=dtype)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype)
    return np.eye(3, dtype=dtype) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


DOWN = np.diag([1.0, -1.0, -1.0])   # camera x right, y = -Y, looking along -Z


class Scene:
    """two cameras over the ground plane z = 0, each tilted by up to 0.2 rad off the nadir"""

    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        self.seed = seed
        self.c1 = np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(90, 110)])
        self.c2 = self.c1 + np.array([rng.uniform(15, 35), rng.uniform(-12, 12), rng.uniform(-5, 5)])
        tilt = lambda: (lambda a: a / np.linalg.norm(a) * rng.uniform(0.02, 0.2))(rng.normal(size=3))
        self.w1, self.w2 = tilt(), tilt()

    def cameras(self, dtype=np.float64):
        D = DOWN.astype(dtype)
        return _rot(self.w1, dtype) @ D, _rot(self.w2, dtype) @ D

    def pixels(self, rng, M, noise, model=MODEL):
        """M ground points seen by both cameras; image-2 pixels with `noise` x focal length of Gaussian noise"""
        R1, R2 = self.cameras()
        px1 = np.stack([rng.uniform(300, 3700, M), rng.uniform(300, 2700, M)], 1)
        u = (px1 - MODEL[1:3]) / MODEL[0]
        d = np.concatenate([u, np.ones((M, 1))], 1) @ R1          # rows: R1^T d
        s = -self.c1[2] / d[:, 2]
        X = self.c1 + s[:, None] * d
        X2 = (X - self.c2) @ R2.T
        u2 = X2[:, :2] / X2[:, 2:3] + noise * rng.normal(size=(M, 2))
        return u * model[0] + model[1:3], u2 * model[0] + model[1:3]

    def homography_ld(self):
        """H = R + t n' / d between the normalised coordinates, from the scene's doubles in long double, h22 = 1"""
        R1, R2 = self.cameras(LD)
        c1, c2 = self.c1.astype(LD), self.c2.astype(LD)
        R = R2 @ R1.T
        t = R2 @ (c1 - c2)
        n = R1 @ np.array([0, 0, 1], LD)
        d = -c1[2]                     # n . X1 for a point of the plane z = 0
        H = R + np.outer(t, n) / d
        return H / H[2, 2]


def _job(family, name, px1, px2, flags, model1=MODEL, model2=MODEL, noisy=True, scene=None):
    return dict(family=family, name=name, px1=np.ascontiguousarray(px1, np.float64).reshape(-1, 2),
                px2=np.ascontiguousarray(px2, np.float64).reshape(-1, 2), flags=np.ascontiguousarray(flags, np.uint8),
                model1=np.array(model1, np.float64), model2=np.array(model2, np.float64), noisy=noisy, scene=scene)


def _scene_job(family, name, seed, M, n_in, noise, where="random", model=MODEL):
    sc = Scene(seed)
    rng = np.random.default_rng(seed + 7919)
    px1, px2 = sc.pixels(rng, M, noise, model)
    if isinstance(where, str):
        idx = dict(random=lambda: np.sort(rng.choice(M, n_in, replace=False)), first=lambda: np.arange(n_in),
                   last=lambda: np.arange(M - n_in, M))[where]()
    else:
        idx = np.asarray(where, np.int64)
    flags = np.zeros(M, np.uint8)
    flags[idx] = 1
    out = flags == 0                   # gross outliers: the image-2 pixel anywhere in the image
    px2[out] = np.stack([rng.uniform(0, 4000, int(out.sum())), rng.uniform(0, 3000, int(out.sum()))], 1) * (model[0] / MODEL[0]) \
        + (model[1:3] - MODEL[1:3] * (model[0] / MODEL[0]))
    return _job(family, name, px1, px2, flags, model, model, noisy=noise > 0, scene=sc)


NOISES = (0.0, 1e-4, 3e-3)
SCENE_SIZES = {4: (4,), 5: (4, 5), 9: (4, 5, 9), 63: (4, 5, 32, 33, 63), 64: (4, 32, 33, 64), 65: (5, 33, 64, 65),
               127: (64, 65, 127), 128: (65, 128), 129: (64, 129), 1200: (4, 65, 600, 1200), 5000: (33, 2500, 5000)}


def scenes():
    jobs, seed = [], 1000
    for M, n_ins in SCENE_SIZES.items():
        for n_in in n_ins:
            for noise in NOISES:
                seed += 1
                jobs.append(_scene_job("scenes", "scenes_M%d_in%d_noise%g" % (M, n_in, noise), seed, M, n_in, noise))
    return jobs


def few():
    jobs = []
    spread = [3, 70, 140, 199]         # one set flag per 64-chunk of the 200 matches
    for n_in in range(5):
        jobs.append(_scene_job("few", "few_M20_in%d" % n_in, 2000 + n_in, 20, n_in, 1e-4, where=[2, 7, 11, 19][:n_in]))
        jobs.append(_scene_job("few", "few_M200_in%d" % n_in, 2010 + n_in, 200, n_in, 1e-4, where=spread[:n_in]))
    jobs.append(_job("few", "few_M0", np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0, np.uint8), noisy=False))
    return jobs


def _scaled(job, name, i, s):
    """correspondence i's coordinates of both images times s"""
    j = dict(job, name=name, px1=job["px1"].copy(), px2=job["px2"].copy(), noisy=True)
    j["px1"][i] = MODEL[1:3] + s * (j["px1"][i] - MODEL[1:3])
    j["px2"][i] = MODEL[1:3] + s * (j["px2"][i] - MODEL[1:3])
    return j


def placement():
    M = 320
    jobs = [_scene_job("placement", "placement_first", 3000, M, 40, 1e-4, where="first"),
            _scene_job("placement", "placement_last", 3000, M, 40, 1e-4, where="last"),
            _scene_job("placement", "placement_every64th", 3000, M, 5, 1e-4, where=np.arange(0, M, 64))]
    base = _scene_job("placement", "", 3000, M, 40, 1e-4, where=np.arange(5, M, 8))
    inl = np.flatnonzero(base["flags"])
    # both rows of one correspondence are pivot rows: its entries are the system's largest by a factor of 8 (x x' by 64)
    jobs.append(_scaled(base, "placement_sibling", inl[17], 8.0))
    jobs.append(_scaled(base, "placement_last_largest", inl[-1], 8.0))
    return jobs


def _survives(k):
    """lattice coordinates k / 8 that come back exactly from the unit ray: (k / 8 / n) / (1 / n) == k / 8 in fp64"""
    p = np.asarray(k, np.float64) / 8
    r = rays_of(p, UNIT)
    return (r[:, 0] / r[:, 2] == p[:, 0]) & (r[:, 1] / r[:, 2] == p[:, 1])


def _lattice(kind, inconsistent):
    k = np.array([(a, b) for a in range(-5, 6) for b in range(-5, 6)])
    k2 = np.stack([-k[:, 1] + 1, k[:, 0] - 1], 1) if kind == "similarity" else np.stack([-k[:, 1], k[:, 0]], 1)
    keep = (np.abs(k2).max(1) <= 5) & _survives(k) & _survives(k2)
    k, k2 = k[keep], k2[keep].copy()
    if inconsistent:
        for step, col in ((7, 0), (11, 1)):
            for i in range(0, len(k2), step):
                for d in (1, -1):
                    cand = k2[i].copy()
                    cand[col] += d
                    if abs(cand[col]) <= 5 and _survives(cand[None])[0]:
                        k2[i] = cand
                        break
    return k / 8.0, k2 / 8.0


def ties():
    jobs = []
    for kind in ("similarity", "rotation90"):
        for inc in (False, True):
            p1, p2 = _lattice(kind, inc)
            jobs.append(_job("ties", "ties_%s%s" % (kind, "_moved" if inc else ""), p1, p2, np.ones(len(p1), np.uint8), UNIT, UNIT,
                             noisy=inc))
    return jobs


def deficient():
    # 40 collinear inliers, noise-free: image-1 y is the principal point's, so y = 0 exactly and three columns vanish
    sc = Scene(4000)
    rng = np.random.default_rng(4001)
    px1, px2 = sc.pixels(rng, 60, 0.0)
    R1, R2 = sc.cameras()

    def project(p1):
        u = (p1 - MODEL[1:3]) / MODEL[0]
        d = np.concatenate([u, np.ones((len(u), 1))], 1) @ R1
        X = sc.c1 + (-sc.c1[2] / d[:, 2])[:, None] * d
        X2 = (X - sc.c2) @ R2.T
        return X2[:, :2] / X2[:, 2:3] * MODEL[0] + MODEL[1:3]

    px1[:40, 1] = MODEL[2]
    px2[:40] = project(px1[:40])
    flags = np.zeros(60, np.uint8)
    flags[:40] = 1
    jobs = [_job("deficient", "deficient_collinear40", px1, px2, flags, noisy=False, scene=sc)]
    # the same on an oblique line: the dependent columns do not vanish, their pivots are roundoff that the rank threshold drops
    px1, px2 = px1.copy(), px2.copy()
    px1[:40, 1] = 900.0 + 0.37 * px1[:40, 0]
    px2[:40] = project(px1[:40])
    jobs.append(_job("deficient", "deficient_collinear40_oblique", px1, px2, flags, noisy=False, scene=sc))
    # four inliers, two of them the same correspondence
    j = _scene_job("deficient", "deficient_repeated_of4", 4010, 20, 4, 0.0, where=[1, 6, 12, 17])
    j["px1"][12], j["px2"][12] = j["px1"][6], j["px2"][6]
    jobs.append(j)
    # every inlier twice
    j = _scene_job("deficient", "deficient_every_inlier_twice", 4020, 40, 40, 1e-4, where="first")
    j["px1"][20:], j["px2"][20:] = j["px1"][:20], j["px2"][:20]
    jobs.append(j)
    return jobs


def extreme():
    base = _scene_job("extreme", "", 5000, 40, 30, 1e-4, where="first", model=UNIT)
    jobs = []

    def add(name, s1, s2):
        with np.errstate(all="ignore"):
            jobs.append(dict(base, name="extreme_" + name, px1=base["px1"] * s1, px2=base["px2"] * s2))

    for s in (1e60, 1e120, 1e-60, 1e-170):
        add("img1_x%g" % s, s, 1.0)
        add("img2_x%g" % s, 1.0, s)
        add("both_x%g" % s, s, s)
    add("2^60_2^-60", 2.0 ** 60, 2.0 ** -60)
    add("2^-60_2^60", 2.0 ** -60, 2.0 ** 60)
    add("1e-200_1e100", 1e-200, 1e100)
    add("1e100_1e-200", 1e100, 1e-200)
    for what, v in (("overflow", 1e200), ("nan", np.nan)):
        for where, i in (("first", 0), ("inlier", 11), ("outlier", 35)):   # (first: the NaN is the first cell of the search)
            j = dict(base, name="extreme_%s_%s" % (what, where), px1=base["px1"].copy())
            j["px1"][i, 0] = v
            jobs.append(j)
    # the lattice unscaled: the row 0 .. 0 1 is never a pivot row, the solution is the zero vector and H = 0 / 0
    p1, p2 = _lattice("similarity", True)
    jobs.append(_job("extreme", "extreme_lattice_unscaled", p1 * 8 * 14, p2 * 8 * 14, np.ones(len(p1), np.uint8), UNIT, UNIT))
    return jobs


FAMILIES = dict(scenes=scenes, few=few, placement=placement, ties=ties, deficient=deficient, extreme=extreme)
_CACHE = {}


def family(name):
    if name not in _CACHE:
        _CACHE[name] = FAMILIES[name]()
    return _CACHE[name]


def all_jobs():
    return [j for f in FAMILIES for j in family(f)]


def prepared(job):
    """rays, the long-double reference and whether the job carries the bound: every job does except the family `extreme`,
    a job whose long-double H is not finite, and a job of noisy data whose fp64 rank is below 9"""
    if "_prep" not in job:
        r1, r2 = job_rays(job)
        ref = reference(r1, r2, job["flags"])
        bound = (job["family"] != "extreme" and bool(np.all(np.isfinite(np.asarray(ref["H"], np.float64))))
                 and not (ref["rank"] < 9 and job["noisy"]))
        job["_prep"] = dict(r1=r1, r2=r2, ref=ref, bound=bound, b=bounds(ref, r1, r2) if bound else None)
    return job["_prep"]


def oracle_rounds(oracle, r1, r2, flags, rounds):
    """`rounds` times fitInliers + evaluate of the oracle from the given flags (relax_group.cpp:158-166): H, the last flags,
    MSAC sum / M"""
    corr = corr7(r1, r2)
    M = len(corr)
    flags = np.asarray(flags, np.uint8)
    for _ in range(rounds):
        H, Hi = oracle.fit_inliers(corr, flags)
        s, flags, _ = oracle.evaluate(corr, H, Hi)
    return H, flags, (s / M if M else 0.0)


def corr7(r1, r2):
    """the oracle's correspondence rows: measurement1, measurement2, quality"""
    return np.ascontiguousarray(np.concatenate([r1, r2, np.zeros((len(r1), 1))], 1))


# ------------------------------------------------------------------------------------------------ minimal samples
def samples(n=2000, seed=6000):
    """n minimal samples (x, y, x', y' of four correspondences, divided by z in fp64) drawn from the `scenes` jobs, inliers
    and outliers alike"""
    rng = np.random.default_rng(seed)
    jobs = [j for j in family("scenes") if len(j["flags"]) >= 4]
    out = np.zeros((n, 16))
    for s in range(n):
        j = jobs[int(rng.integers(len(jobs)))]
        idx = rng.choice(len(j["flags"]), 4, replace=False)
        r1, r2 = rays_of(j["px1"][idx], j["model1"]), rays_of(j["px2"][idx], j["model2"])
        out[s] = np.stack(coords(r1, r2, np.float64), 1).ravel()
    return out


def special_samples():
    """(name, xy16, bounded): the tied, repeated, collinear, extreme and NaN samples"""
    out = []
    p1, p2 = _lattice("similarity", True)
    q1, q2 = _lattice("rotation90", False)
    pick = [0, 6, len(p1) // 2, len(p1) - 1]      # the 7th point is a moved one
    out.append(("tied_moved", np.concatenate([p1[pick], p2[pick]], 1).ravel(), True))
    pick = [0, 5, len(q1) // 2 + 1, len(q1) - 2]
    out.append(("tied_rotation", np.concatenate([q1[pick], q2[pick]], 1).ravel(), True))
    base = samples(4, seed=6100)
    rep = base[0].copy()
    rep[8:12] = rep[4:8]
    out.append(("repeated", rep, True))
    col = base[1].reshape(4, 4).copy()
    col[2, :2] = 0.5 * (col[0, :2] + col[1, :2])  # the third image-1 point between the first two
    out.append(("collinear", col.ravel(), True))
    col3 = base[1].reshape(4, 4).copy()
    col3[:, 1] = 0.25                              # all four on one line, exactly
    out.append(("collinear_all", col3.ravel(), True))
    for s in (1e60, 1e120, 1e-170):
        e = base[2].reshape(4, 4).copy()
        e[:, :2] *= s
        out.append(("extreme_img1_x%g" % s, e.ravel(), False))
    e = base[2].reshape(4, 4).copy()
    e[:, :2] *= 2.0 ** 60
    e[:, 2:] *= 2.0 ** -60
    out.append(("extreme_2^60_2^-60", e.ravel(), False))
    for v, nm in ((np.nan, "nan"), (np.inf, "inf")):
        for pos in (0, 14):
            e = base[3].copy()
            e[pos] = v
            out.append(("%s_at%d" % (nm, pos), e, False))
    return out


def sample_bound(ref):
    """bounded samples: the long-double H finite and the fp64 rank full (a minimal sample has no redundancy: below rank 9
    the truncated solution is whatever the roundoff of the last pivots makes of it)"""
    return bool(np.all(np.isfinite(np.asarray(ref["H"], np.float64)))) and ref["rank"] == 9

"""Scenes, an 80-bit long-double reference and the bounds for the two fp64 device steps of the dense stage that no raw test
named before: dense_predict_kernel (observed through ochip_dense_link's slot rows) and dense_triangulate_kernel /
dense_triangulate_large_kernel (ochip_dense_triangulate), csrc/dense.hip.  Data and arithmetic only; numpy, deterministic, no
device.  tests/test_dense_kernel_fixtures.py checks the fixtures themselves on the CPU, tests/test_gpu_dense_kernels.py runs
the device against them.

One set of statements, two precisions.  rotate(), project(), intersect() and the track rule below are written once, in the
order of the kernel's statements, on whatever dtype their arguments have: on np.longdouble they are the reference, on float64
they are the restatement of the kernel (predict_fp64, tri_fp64) that the CPU test holds against the reference and that the
mutations are applied to.  numpy has no fused multiply-add, the library is built with -ffp-contract=off.

Predict.  Every scene is built so that each in-image candidate is certain to be accepted: image c has a feature for ground
point j iff the long-double projection of P_j into c lies in [0, cols) x [0, rows), the feature sits at that projection rounded
to fp64, descriptors are distinct per point and carry no bit flips, and a feature's hit is its own P_j.  The twin is then in
the 150 px disc at Hamming distance 0 (one candidate: 0 < 0.35; more: 0 < 0.85 * second, second > 0), so the slot row of a
feature is the twin's measurement id in every in-image camera among the 11 smallest (d^2, index), the source skipped,
0xFFFFFFFF behind them; counts2[0] = counts2[1] = the number of such candidates; the roots are a plain union-find's.
Margins (reference only; the exact families need none): a point is dropped when a projection comes within BORDER_MARGIN px
of an image border or two consecutive cameras of its ordered list, up to rank 12, differ by less than ORDER_MARGIN relative
in d^2.  At most DROP_CAP of a scene's points may go.

Triangulate.  A track is a list of (image, pixel) members made for it; the index of a scene holds exactly the members of its
tracks.  Rays of undistorted cameras are long double from the pixel on; rays of distorted cameras start from the oracle's
fp64 image_to_3d (held bit-equal to the device's elsewhere; the iterative inverse is not the subject) and go on in long
double.  Then the closed-form midpoint of the first two members' rays, the reprojection with the 1e-3 clamp and the forward
lens model, e^2 <= 64, and - when not every member is an inlier - the midpoint again from the first two inliers.
valid is compared exactly; a valid point is held to
    |p - p_ref|_inf <= C_TRI 2^-53 kappa scale,   kappa = n11 n22 / |denom| of the pair that produced the point,
                                                    scale = max(|o1|_inf, |o2|_inf, |p_ref|_inf).
Margins (reference only): a generated track is dropped when an intersection it takes has |denom| in (0, 1e-6] or |t| or |s|
below 1e-6 scale, when a member's reprojection error is within 1e-6 px of 8, or when the bound of the first point times
f / z of any member reaches 1e-7 px.  A denom of exactly 0 (the exact family: equal and opposite directions from identity-
oriented cameras with integer geometry, 0 in fp64 and in long double alike) is outside (0, 1e-6] and stays.  A first pair
from one image has equal origins, t = s = 0, and falls to the |t| margin: no such track is kept.  At most DROP_CAP of the
generated tracks may go.

C_TRI = 2^3.  Calibrated in tests/test_dense_kernel_fixtures.py on the CPU: the fp64 numpy restatement against the long-
double reference over every track of every scene here (282 valid tracks); worst ratio error / (2^-53 kappa scale) = 3.73
(track "tri2/bulk11", two undistorted cameras), twice that rounded up to a power of two.  That figure is the CPU's.  The
device's own worst ratio is printed by the GPU test (DENSE_TRI_RATIOS) and recorded in DESIGN.md.

The mutation `abs dropped from the denom test` has no input that tells it from the kernel: denom = n11 n22 - n12^2 is a
Gram determinant, never negative but by rounding, and with the unit directions of any camera that rounding is 1e-16 against
the threshold's 1e-9.  An input on which `denom > 1e-9` and `|denom| > 1e-9` differ has a denom whose sign is wrong, so the
kernel's own point is noise there and no reference agrees with it.  The CPU test asserts the equivalence over the fixtures
(EQUIVALENT_MUTATIONS) instead of pretending to catch it."""
import functools

import numpy as np

from opencalibration_amd import synth

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, (
    "numpy.longdouble is not the 80-bit extended type here (eps %g): the long-double dense reference needs a 64-bit "
    "significand" % np.finfo(LD).eps)

U = 2.0 ** -53
NONE = 0xFFFFFFFF
DENSE_K = 11                 # MAX_CANDIDATE_IMAGES + 1
CELL, RADIUS = 151.0, 150.0
DESCRIPTOR_BITS, RATIO, MAX_ABS = 486, 0.85, 0.35
MAX_REPROJECTION = 8.0
TRI_LARGE = 32               # tracks above this many members go to the wavefront kernel
BORDER_MARGIN, ORDER_MARGIN = 1e-6, 1e-12
DROP_CAP = 0.01
C_TRI = 2.0 ** 3             # calibration: tests/test_dense_kernel_fixtures.py
W, H, F = 1000.0, 750.0, 750.0
DIST_A = (0.02, -0.07, 0.1, 1e-4, -2e-4)
DIST_B = (-0.05, 0.01, -0.002, 1e-3, -5e-4)
Q_DOWN = np.array([1.0, 0.0, 0.0, 0.0])      # rotation by pi about x: the camera looks down
Q_IDENTITY = np.array([0.0, 0.0, 0.0, 1.0])

PREDICT_MUTATIONS = ("tie_high", "ten_nearest", "keep_source", "gt_cols", "no_clamp", "no_k2")
TRI_MUTATIONS = ("second_from_members", "lane_second", "lane_first_only", "no_sign_rule", "no_clamp", "no_k2", "max_err_wide", "max_err_narrow")
EQUIVALENT_MUTATIONS = ("no_abs_denom",)


def model10(distortion=None, f=F, w=W, h=H):
    m = np.array([f, w / 2, h / 2, 0, 0, 0, 0, 0, w, h], np.float64)
    if distortion is not None:
        m[3:8] = distortion
    return m


def conj(q):
    return np.asarray(q) * np.array([-1.0, -1.0, -1.0, 1.0])


# ------------------------------------------------------------------------------------- the kernel's statements, any dtype
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def rotate(q, v):
    """drotate: Eigen's QuaternionBase::_transformVector, v + 2 w (qv x v) + qv x 2 (qv x v)"""
    qv, w = q[..., :3], q[..., 3:4]
    uv = _cross(qv, v)
    uv = uv + uv
    c = _cross(qv, uv)
    return (v + uv * w) + c


def project(point, pos, q_inv, model, clamp=True, k2=True):
    """dense_project: image_from_3d(point, model, position, orientation) with the z < 1e-3 clamp"""
    r = rotate(q_inv, point - pos)
    z = r[..., 2]
    if clamp:
        z = np.where(z < 1e-3, z.dtype.type(1e-3), z)
    p = (r[..., 0] / z, r[..., 1] / z)
    r20 = p[0] * p[0] + p[1] * p[1]
    r21 = r20 * r20
    r22 = r21 * r20
    if k2:
        radial = model[..., 3] * r20 + model[..., 4] * r21 + model[..., 5] * r22
    else:
        radial = model[..., 3] * r20 + model[..., 5] * r22
    prod = p[0] * p[1]
    out = []
    for i in range(2):
        d = (1.0 + radial) * p[i] + 2.0 * prod * model[..., 6 + i] + model[..., 7 - i] * (r20 + 2.0 * p[i] * p[i])
        out.append(d * model[..., 0] + model[..., 1 + i])
    return np.stack(out, -1)


def inside_image(px, model, gt=False):
    """the complement of the kernel's skip test `px < 0 || px >= cols || py < 0 || py >= rows` ((mutant) gt: `>`)"""
    x, y, cols, rows = px[..., 0], px[..., 1], model[..., 8], model[..., 9]
    with np.errstate(invalid="ignore"):
        if gt:
            return ~((x < 0) | (x > cols) | (y < 0) | (y > rows))
        return ~((x < 0) | (x >= cols) | (y < 0) | (y >= rows))


def _dist2(pos, P):
    dx, dy, dz = pos[None, :, 0] - P[:, None, 0], pos[None, :, 1] - P[:, None, 1], pos[None, :, 2] - P[:, None, 2]
    return dx * dx + dy * dy + dz * dz


# --------------------------------------------------------------------------------------------------- the index layout
def index_arrays(features):
    """ochip_dense_index_create's arguments for per-image (loc [k][2], desc [k][8]): every image's features sorted by the cell
    of a uniform grid, the cell start tables, and id_of_pos (measurement id = image offset + number in the ORIGINAL order)"""
    feat_off, cell_off, grid2, origin2, cell_start, sdesc, sloc, ids = [0], [0], [], [], [], [], [], []
    for loc, d in features:
        assert len(loc) > 0
        ox, oy = np.floor(loc.min(0))
        ncx, ncy = int((loc[:, 0].max() - ox) // CELL) + 1, int((loc[:, 1].max() - oy) // CELL) + 1
        c = (np.floor((loc[:, 1] - oy) / CELL) * ncx + np.floor((loc[:, 0] - ox) / CELL)).astype(int)
        perm = np.argsort(c, kind="stable")
        cell_start.append(np.searchsorted(c[perm], np.arange(ncx * ncy + 1)).astype(np.uint32))
        sdesc.append(d[perm]), sloc.append(loc[perm]), ids.append(feat_off[-1] + perm)
        grid2 += [ncx, ncy]
        origin2 += [ox, oy]
        feat_off.append(feat_off[-1] + len(loc))
        cell_off.append(cell_off[-1] + ncx * ncy + 1)
    return dict(n_images=len(features), total=feat_off[-1], feat_off=np.array(feat_off, np.uint64),
                desc=np.ascontiguousarray(np.concatenate(sdesc), np.uint64), loc=np.ascontiguousarray(np.concatenate(sloc), np.float64),
                cell_off=np.array(cell_off, np.uint64), cell_start=np.ascontiguousarray(np.concatenate(cell_start)),
                grid2=np.array(grid2, np.int32), origin2=np.array(origin2, np.float64),
                id_of_pos=np.ascontiguousarray(np.concatenate(ids), np.uint32))


def cams17(pos, q, models):
    """the kernel's camera records: position, inverse orientation, model"""
    out = np.zeros((len(pos), 17))
    out[:, 0:3], out[:, 3:7], out[:, 7:17] = pos, conj(q), models
    return out


def union_roots(total, rows_by_id):
    """root per measurement id of a plain union-find over (id, row entry) pairs: the smallest id of the component for a
    measurement some match names, 0xFFFFFFFF for the others"""
    parent = list(range(total))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    matched = np.zeros(total, bool)
    for a in range(total):
        for b in rows_by_id[a]:
            if b == NONE:
                continue
            b = int(b)
            matched[a] = matched[b] = True
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) if matched[i] else NONE for i in range(total)], np.uint32)


# ============================================================================================================ predict
def _build_predict(name, family, pos, q, models, P, exact=False, seed=0):
    """the scene of ground points P over the cameras: features, hits and everything expected, from the long-double projection"""
    pos, q, models, P = [np.ascontiguousarray(a, np.float64) for a in (pos, q, models, P)]
    n = len(pos)
    posL, qiL, modL = pos.astype(LD), conj(q).astype(LD), models.astype(LD)

    def reference(P):
        PL = P.astype(LD)
        px = project(PL[:, None, :], posL[None], qiL[None], modL[None])
        return px, inside_image(px, modL[None]), _dist2(posL, PL)

    px, inside, d2 = reference(P)
    P = P[inside.any(1)]                         # a point no camera sees is no point of the scene
    px, inside, d2 = reference(P)
    generated = len(P)
    if not exact:
        border = np.minimum(np.minimum(np.abs(px[..., 0]), np.abs(px[..., 0] - modL[None, :, 8])),
                            np.minimum(np.abs(px[..., 1]), np.abs(px[..., 1] - modL[None, :, 9]))).min(1) < BORDER_MARGIN
        sd = np.sort(d2, 1)[:, :12]
        close = ((sd[:, 1:] - sd[:, :-1]) < ORDER_MARGIN * sd[:, 1:]).any(1)
        P = P[~(border | close)]
        px, inside, d2 = reference(P)
    m = len(P)
    order = np.argsort(d2, axis=1, kind="stable")            # (d^2, index): the lower index wins a tie
    desc = synth.descriptors_for_ids(np.arange(m, dtype=np.int64) + 100000 * (seed + 1))
    assert len({d.tobytes() for d in desc}) == m
    feat_id = np.full((m, n), -1, np.int64)
    features, off = [], 0
    for c in range(n):
        js = np.nonzero(inside[:, c])[0]
        assert len(js), "%s: image %d sees nothing" % (name, c)
        feat_id[js, c] = off + np.arange(len(js))
        features.append((np.ascontiguousarray(px[js, c].astype(np.float64)), np.ascontiguousarray(desc[js])))
        off += len(js)
    total = off
    f_pt, f_img = [a[np.argsort(feat_id[np.nonzero(feat_id >= 0)])] for a in np.nonzero(feat_id >= 0)]
    nohit = np.arange(total) % 17 == 5
    hits = P[f_pt].copy()
    hits[nohit, 0] = np.nan
    s = dict(name=name, family=family, exact=exact, pos=pos, q=q, models=models, P=P, n_images=n, total=total, generated=generated,
             dropped=generated - m, features=features, feat_id=feat_id, f_pt=f_pt, f_img=f_img, nohit=nohit, hits_by_id=hits,
             ref_px=px, ref_inside=inside, ref_d2=d2, ref_order=order)
    s["exp_slot_by_id"], _ = _slot_rows(s, order, inside, DENSE_K, True)
    s["exp_root"] = union_roots(total, s["exp_slot_by_id"])
    s["exp_queries"] = int((s["exp_slot_by_id"] != NONE).sum())
    return s


def _slot_rows(s, order, inside, take, skip_source):
    rows = np.full((s["total"], DENSE_K), NONE, np.uint32)
    feat_id, queries = s["feat_id"], 0
    for k in range(s["total"]):
        if s["nohit"][k]:
            continue
        j, src, used = s["f_pt"][k], s["f_img"][k], 0
        for c in order[j, :take]:
            if (skip_source and c == src) or not inside[j, c]:
                continue
            rows[k, used] = feat_id[j, c] if feat_id[j, c] >= 0 else NONE     # (a mutant's candidate without a twin: a used slot, no match)
            used += 1
        queries += used
    return rows, queries


def predict_fp64(s, mutation=None):
    """dense_predict_kernel restated in fp64: (slot rows by id, queries, matches, roots).  The 11 smallest (d, index) are the
    same whatever order the cameras are met in, so the restatement sorts.  The disc search is not restated: a candidate's
    match is its twin (0xFFFFFFFF where a mutant's candidate has none)."""
    assert mutation is None or mutation in PREDICT_MUTATIONS, mutation
    pos, qi, models, P = s["pos"], conj(s["q"]), s["models"], s["P"]
    d2 = _dist2(pos, P)
    idx = np.broadcast_to(np.arange(s["n_images"]), d2.shape)
    order = np.lexsort((-idx if mutation == "tie_high" else idx, d2), axis=1)
    with np.errstate(all="ignore"):
        px = project(P[:, None, :], pos[None], qi[None], models[None], clamp=mutation != "no_clamp", k2=mutation != "no_k2")
    inside = inside_image(px, models[None], gt=mutation == "gt_cols")
    rows, queries = _slot_rows(s, order, inside, DENSE_K - 1 if mutation == "ten_nearest" else DENSE_K, mutation != "keep_source")
    return rows, queries, int((rows != NONE).sum()), union_roots(s["total"], rows)


def by_position(s, ix):
    """the scene's per-id arrays in the index's order: (hits [total][3], expected slot rows [total][11])"""
    ids = ix["id_of_pos"]
    return np.ascontiguousarray(s["hits_by_id"][ids]), s["exp_slot_by_id"][ids]


def _ground(x, y):
    return 1e-3 * x + 1e-2 * y + 1.5 * np.sin(x / 40.0) * np.cos(y / 55.0)


def _survey(rng, n, cols, spacing=(46.0, 45.0), height=100.0):
    """cameras as in dense_fixtures.dense_scene: a jittered grid, yawed and tilted, looking down"""
    r_idx, c_idx = np.divmod(np.arange(n), cols)
    pos = np.stack([c_idx * spacing[0] + rng.uniform(-1, 1, n), r_idx * spacing[1] + rng.uniform(-1, 1, n),
                    height + rng.uniform(-2, 2, n)], -1)
    yaw, tilt = rng.normal(0, 0.2, n), rng.normal(0, 0.03, (n, 2))
    q = np.stack([tilt[:, 0] / 2, tilt[:, 1] / 2, np.sin(yaw / 2), np.cos(yaw / 2)], -1)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return pos, synth.quat_mul(q, Q_DOWN[None, :])


def _ground_points(rng, pos, count, reach=(0.5 * 100 * W / F, 0.5 * 100 * H / F)):
    gx = rng.uniform(pos[:, 0].min() - reach[0], pos[:, 0].max() + reach[0], count)
    gy = rng.uniform(pos[:, 1].min() - reach[1], pos[:, 1].max() + reach[1], count)
    return np.stack([gx, gy, _ground(gx, gy)], -1)


COUNT_SIZES = (11, 12, 13, 14, 15, 30)


def _lattice(nx, ny, step, height, holes=()):
    xy = [(step * i, step * j) for j in range(ny) for i in range(nx) if (i, j) not in holes]
    pos = np.array([[x, y, height] for x, y in xy], np.float64)
    return pos, np.tile(Q_DOWN, (len(pos), 1))


EXACT_MODEL = np.array([512.0, 512.0, 384.0, 0, 0, 0, 0, 0, 1024.0, 768.0])   # at depth 64: px = 8 dx + 512, py = -8 dy + 384


@functools.lru_cache(None)
def predict_scenes():
    out = []
    # camera counts: one candidate fewer than slots (11), every n % 4 (12 .. 15), a real choice (30)
    for n in COUNT_SIZES:
        rng = np.random.default_rng(4100 + n)
        pos, q = _survey(rng, n, 6 if n == 30 else 4)
        out.append(_build_predict("count%d" % n, "counts", pos, q, np.tile(model10(), (n, 1)), _ground_points(rng, pos, 110), seed=n))
    # the source outside the nearest 11: cameras 15 m apart, 133 m x 100 m footprints
    rng = np.random.default_rng(4201)
    pos, q = _survey(rng, 40, 8, spacing=(15.0, 15.0))
    out.append(_build_predict("far40", "far", pos, q, np.tile(model10(), (40, 1)), _ground_points(rng, pos, 50), seed=41))
    # lens distortion, the two sets the suite uses
    for k, dist in enumerate((DIST_A, DIST_B)):
        rng = np.random.default_rng(4300 + k)
        pos, q = _survey(rng, 13 + k, 4)
        out.append(_build_predict("distortion_%s" % "ab"[k], "distortion", pos, q, np.tile(model10(dist), (13 + k, 1)),
                                  _ground_points(rng, pos, 160), seed=50 + k))
    # exact ties: an integer lattice at one height with holes (ties of 2, 3 and 4, across rank 11 too), points at integer and
    # half-integer coordinates; everything is exact in fp64, no margins
    rng = np.random.default_rng(4400)
    pos, q = _lattice(6, 5, 16.0, 64.0, holes=((1, 1), (4, 3), (2, 3)))
    centres = [(8.0 + 16 * i, 8.0 + 16 * j) for i in range(5) for j in range(4)]
    mids = [(8.0 + 16 * i, 16.0 * j) for i in range(5) for j in range(5)] + [(16.0 * i, 8.0 + 16 * j) for i in range(6) for j in range(4)]
    nodes = [(16.0 * i, 16.0 * j) for i in range(6) for j in range(5)]
    pick = lambda lst, k: [lst[i] for i in rng.choice(len(lst), k, replace=False)]
    xy = pick(centres, 14) + pick(mids, 14) + pick(nodes, 8) + [(x, y) for x, y in zip(rng.integers(-16, 193, 24) / 2.0, rng.integers(-16, 145, 24) / 2.0)]
    P = np.array([[x, y, 0.0] for x, y in dict.fromkeys(xy)])
    out.append(_build_predict("ties_lattice", "ties", pos, q, np.tile(EXACT_MODEL, (len(pos), 1)), P, exact=True, seed=60))
    # exact borders: 12 lattice cameras, integer points out to where a projection is exactly 0.0 (inside) or exactly cols / rows
    rng = np.random.default_rng(4401)
    pos, q = _lattice(4, 3, 16.0, 64.0)
    xy = [(cx + sx * 64.0, float(rng.integers(-10, 40))) for cx in (0.0, 16.0, 32.0, 48.0) for sx in (-1, 1)]
    xy += [(float(rng.integers(-10, 58)), cy + sy * 48.0) for cy in (0.0, 16.0, 32.0) for sy in (-1, 1)]
    xy += [(float(x), float(y)) for x, y in zip(rng.integers(-70, 120, 60), rng.integers(-55, 90, 60))]
    P = np.array([[x, y, 0.0] for x, y in dict.fromkeys(xy)])
    out.append(_build_predict("ties_borders", "ties", pos, q, np.tile(EXACT_MODEL, (len(pos), 1)), P, exact=True, seed=61))
    # the clamp: 8 cameras near 100 m with points within millimetres of their planes (below by less than 1e-3, above, and
    # just past the clamp), 6 cameras near 150 m that see those points from above
    rng = np.random.default_rng(4500)
    low = np.stack([rng.uniform(0, 40, 8), rng.uniform(0, 30, 8), 100 + rng.uniform(-2, 2, 8)], -1)
    up, q_up = _survey(rng, 6, 3, spacing=(15.0, 15.0), height=150.0)
    up[:, :2] += [5.0, 7.0]
    _, q_low = _survey(rng, 8, 4)
    pos, q = np.concatenate([low, up]), np.concatenate([q_low, q_up])
    pts, kinds = [], []
    for c in range(8):
        R = synth.quat_to_matrix(q[c])
        for k in range(12):
            z = [rng.uniform(1e-5, 9.9e-4), rng.uniform(-2e-3, -1e-5), rng.uniform(1.5e-3, 4e-3)][k % 3]
            sc = max(z, 1e-3) / 1e-3
            pts.append(pos[c] + R @ np.array([rng.uniform(-6e-4, 6e-4) * sc, rng.uniform(-4e-4, 4e-4) * sc, z]))
    P = np.concatenate([np.array(pts), _ground_points(rng, pos, 60, reach=(20.0, 15.0))])
    out.append(_build_predict("clamp", "clamp", pos, q, np.tile(model10(), (14, 1)), P, seed=70))
    return out


def predict_facts(s):
    """what a predict scene contains, from the reference: the coverage the CPU test asserts"""
    n, order, inside, d2 = s["n_images"], s["ref_order"], s["ref_inside"], s["ref_d2"]
    live = ~s["nohit"]
    rank_of_src = np.array([int(np.nonzero(order[j] == c)[0][0]) for j, c in zip(s["f_pt"], s["f_img"])])
    row_len = (s["exp_slot_by_id"] != NONE).sum(1)
    sd = np.take_along_axis(d2, order, 1)
    ties = {2: 0, 3: 0, 4: 0}
    for row in sd[:, :DENSE_K]:
        _, cnt = np.unique(row, return_counts=True)
        for c in cnt:
            if c in ties:
                ties[int(c)] += 1
    across = 0
    if n > DENSE_K:
        for j in range(len(sd)):
            a, b = order[j, DENSE_K - 1], order[j, DENSE_K]
            across += bool(sd[j, DENSE_K - 1] == sd[j, DENSE_K] and (inside[j, a] or inside[j, b]))
    px = s["ref_px"]
    qiL = conj(s["q"]).astype(LD)
    z = rotate(qiL[None], s["P"].astype(LD)[:, None, :] - s["pos"].astype(LD)[None])[..., 2]
    near = np.zeros_like(inside)
    near[np.arange(len(order))[:, None], order[:, :DENSE_K]] = True
    return dict(features=s["total"], sources={int(c) for c in s["f_img"][live]}, full_rows=int((row_len[live] == DENSE_K).sum()),
                src_outside=int((rank_of_src[live] >= DENSE_K).sum()), no_hit=int(s["nohit"].sum()),
                out_of_image_candidates=int((near & ~inside).sum()), ties=ties, ties_across_rank_11=across,
                exactly_zero=int(((px[..., 0] == 0) & inside & near).sum() + ((px[..., 1] == 0) & inside & near).sum()),
                exactly_cols=int(((px[..., 0] == s["models"][None, :, 8]) & near).sum() + ((px[..., 1] == s["models"][None, :, 9]) & near).sum()),
                clamped_inside=int(((z < 1e-3) & inside & near).sum()), clamped_above=int(((z < 0) & inside & near).sum()),
                clamped_outside=int(((z < 1e-3) & ~inside & near).sum()))


# ======================================================================================================== triangulate
def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def intersect(d1, o1, d2, o2, mutation=None):
    """dense_ray_intersection and the caller's verdict `finite && !(err < 0)`, in the dtype of the arguments"""
    n11, n12, n22 = _dot(d1, d1), _dot(d1, d2), _dot(d2, d2)
    denom = n11 * n22 - n12 * n12
    out = dict(n11=n11, n22=n22, denom=denom, computed=False, ok=False, point=None, t=None, s=None, o1=o1, o2=o2)
    if not ((denom if mutation == "no_abs_denom" else abs(denom)) > 1e-9):
        return out
    off = o1 - o2
    od1, od2 = _dot(off, d1), _dot(off, d2)
    with np.errstate(all="ignore"):
        t = (n12 * od2 - n22 * od1) / denom
        s = (n11 * od2 - n12 * od1) / denom
        p1, p2 = o1 + d1 * t, o2 + d2 * s
        mid = (p1 + p2) * 0.5
        g = p1 - p2
        err = _dot(g, g) * (1 if (t >= 0 and s >= 0) or mutation == "no_sign_rule" else -1)
    out.update(computed=True, t=t, s=s, point=mid, ok=bool(np.isfinite(mid).all() and not err < 0))
    return out


def _ray(cams, img, px, dtype, image_to_3d):
    """the member's ray and origin.  Long double on an undistorted camera: (px - pp) / f, homogeneous().normalized(), all of
    it long double.  Otherwise the fp64 image_to_3d (the oracle's), carried on in dtype."""
    model = cams["models"][img]
    if dtype is LD and not model[3:8].any():
        x, y = (LD(px[0]) - model[1]) / model[0], (LD(px[1]) - model[2]) / model[0]
        n = np.sqrt(x * x + y * y + 1)
        r = np.array([x / n, y / n, 1 / n], LD)
    else:
        r = image_to_3d(np.array([px], np.float64), np.ascontiguousarray(model))[0].astype(dtype)
    return rotate(cams["q"][img].astype(dtype), r), cams["pos"][img].astype(dtype)


def _two_inliers(inl, n, mutation):
    """the members of the second intersection.  Above TRI_LARGE members as the wavefront kernel finds them: lane i % 64 keeps
    its first two inliers, f0 = the smallest first, f1 = the smallest of (the second of f0's lane, the others' firsts)."""
    idx = np.nonzero(inl)[0]
    if mutation == "second_from_members":
        return 0, 1
    if n <= TRI_LARGE:
        return int(idx[0]), int(idx[1])
    first, second = np.full(64, NONE, np.int64), np.full(64, NONE, np.int64)
    for i in idx:
        if first[i % 64] == NONE:
            first[i % 64] = i
        elif second[i % 64] == NONE:
            second[i % 64] = i
    f0 = first.min()
    if mutation == "lane_second":
        f1 = second.min()
    elif mutation == "lane_first_only":
        f1 = np.where(first == f0, NONE, first).min()
    else:
        f1 = np.where(first == f0, second, first).min()
    return int(f0), int(f1)


def eval_track(cams, images, px, dtype, image_to_3d, mutation=None):
    """triangulateTrack as the kernels run it, in dtype: dict(valid, point, pair, first, second, e2, inliers, depth)"""
    n = len(images)
    res = dict(valid=False, point=None, pair=None, first=None, second=None, e2=None, inliers=None, depth=None, final=None)
    if n < 2:
        return res
    ray = lambda k: _ray(cams, images[k], px[k], dtype, image_to_3d)
    (d1, o1), (d2, o2) = ray(0), ray(1)
    first = res["first"] = intersect(d1, o1, d2, o2, mutation)
    if not first["ok"]:
        return res
    M = first["point"]
    pos, qi, models = cams["pos"][images].astype(dtype), conj(cams["q"][images]).astype(dtype), cams["models"][images].astype(dtype)
    with np.errstate(all="ignore"):
        re = project(M[None], pos, qi, models, clamp=mutation != "no_clamp", k2=mutation != "no_k2")
        ex, ey = re[:, 0] - px[:, 0], re[:, 1] - px[:, 1]
        e2 = ex * ex + ey * ey
        limit = {"max_err_wide": 66.0, "max_err_narrow": 62.0}.get(mutation, MAX_REPROJECTION * MAX_REPROJECTION)
        inl = e2 <= limit
    z = rotate(qi, M[None] - pos)[:, 2]
    res.update(e2=e2, inliers=inl, depth=np.where(z < 1e-3, dtype(1e-3), z))
    if inl.sum() < 2:
        return res
    final, pair = first, (0, 1)
    if inl.sum() < n:
        f0, f1 = _two_inliers(inl, n, mutation)
        if f1 >= n:                      # (a mutant without a second member: the kernel would read past the track)
            return res
        (d1, o1), (d2, o2) = ray(f0), ray(f1)
        final = res["second"] = intersect(d1, o1, d2, o2, mutation)
        pair = (f0, f1)
        if not final["ok"]:
            return res
    res.update(valid=True, point=final["point"], pair=pair, final=final)
    return res


def _scale_of(I, point):
    return float(max(np.max(np.abs(I["o1"])), np.max(np.abs(I["o2"])), np.max(np.abs(point))))


def point_bound(ref, C=C_TRI):
    """C 2^-53 kappa scale of a valid reference result, and (kappa, scale)"""
    I = ref["final"]
    kappa, scale = float(I["n11"] * I["n22"] / abs(I["denom"])), _scale_of(I, ref["point"])
    return C * U * kappa * scale, kappa, scale


def margin_reasons(cams, images, ref):
    """why the reference's decisions on this track are not safe from fp64 rounding (empty: they are)"""
    why = []
    for I in (ref["first"], ref["second"]):
        if I is None:
            continue
        if 0 < abs(I["denom"]) <= 1e-6:
            why.append("denom")
        if I["computed"]:
            sc = _scale_of(I, I["point"])
            if abs(I["t"]) < 1e-6 * sc or abs(I["s"]) < 1e-6 * sc:
                why.append("t or s")
    if ref["e2"] is not None:
        if np.any(np.abs(np.sqrt(ref["e2"]) - MAX_REPROJECTION) <= 1e-6):
            why.append("reprojection at 8 px")
        I = ref["first"]
        b = C_TRI * U * float(I["n11"] * I["n22"] / abs(I["denom"])) * _scale_of(I, I["point"])
        if np.any(b * cams["models"][images, 0] / ref["depth"].astype(np.float64) >= 1e-7):
            why.append("sensitivity")
    return why


TRACK_SIZES = (2, 3, 31, 32, 33, 63, 64, 65, 129, 200)
SECOND_PAIRS = ((0, 1), (0, 2), (1, 2), (5, 6))
LANE_PAIRS = ((5, 69), (5, 70))
HIGH, LOW = 140.0, 70.0


def _tri_cameras(rng, n, distortions):
    """n cameras over one patch of ground, even ones near 140 m and odd ones near 70 m (a gap between two rays is then an
    inlier's error in the one and an outlier's in the other); from 3 cameras on the last one sits 1.5 m beside camera 0"""
    r_idx, c_idx = np.divmod(np.arange(n), 6)
    pos = np.stack([c_idx * 7.0 + rng.uniform(-1, 1, n), r_idx * 7.0 + rng.uniform(-1, 1, n),
                    np.where(np.arange(n) % 2 == 0, HIGH, LOW) + rng.uniform(-2, 2, n)], -1)
    if n <= 3:
        pos[1, :2] = [30.0, 4.0]
    if n >= 3:
        pos[n - 1] = pos[0] + [1.5, 0.2, 0.1]
    yaw, tilt = rng.normal(0, 0.2, n), rng.normal(0, 0.03, (n, 2))
    q = np.stack([tilt[:, 0] / 2, tilt[:, 1] / 2, np.sin(yaw / 2), np.cos(yaw / 2)], -1)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    models = np.stack([model10(distortions[i % len(distortions)]) for i in range(n)])
    return dict(pos=pos, q=synth.quat_mul(q, Q_DOWN[None, :]), models=models, n=n)


class _TrackMaker:
    def __init__(self, cams, seed, image_to_3d, focal=F):
        self.cams, self.rng, self.i3d, self.focal = cams, np.random.default_rng(seed), image_to_3d, focal
        self.n = cams["n"]
        self.high = [i for i in range(self.n) if cams["pos"][i, 2] > 100]
        self.low = [i for i in range(self.n) if cams["pos"][i, 2] <= 100]
        self.centre = cams["pos"][:, :2].mean(0)
        self.turn = 0

    def proj(self, X, img, clamp=True):
        c = self.cams
        return project(np.asarray(X, np.float64), c["pos"][img], conj(c["q"][img]), c["models"][img], clamp=clamp)

    def ground_point(self):
        x, y = self.centre + self.rng.uniform(-15, 15, 2)
        return np.array([x, y, self.rng.uniform(-3, 3)])

    def images_for(self, count):
        """images in turn, so that every image gets members and a long track meets each image many times"""
        out = [(self.turn + k) % self.n for k in range(count)]
        self.turn += count
        return out

    def _epipolar_normal(self, img, other, P):
        """unit pixel direction in img across the epipolar line of other's ray to P"""
        d = P - self.cams["pos"][other]
        e = self.proj(P + 0.05 * d, img) - self.proj(P, img)
        e /= np.linalg.norm(e)
        return np.array([-e[1], e[0]])

    def first_pair(self, kind, pair=None, P=None):
        """(images, pixels, P) of members 0 and 1.  in_in: both observe P; in_out / out_in: the lower camera's pixel is moved
        across the epipolar line so that the midpoint is an inlier's 5 px from the higher camera's ray and an outlier's 10 px
        from the lower one's; out_out: the same with a gap that makes both outliers; behind: the rays diverge in front of the cameras; behind_one: the higher
        camera looks straight down, the lower one away from it - their nearest points lie in front of the one, behind the other"""
        rng, pos, F = self.rng, self.cams["pos"], self.focal
        P = self.ground_point() if P is None else np.asarray(P, np.float64)
        if pair is not None:
            i0, i1 = pair
        elif kind in ("in_out", "out_in", "behind_one"):
            hi, lo = int(rng.choice(self.high)), int(rng.choice(self.low))
            while np.linalg.norm(pos[hi, :2] - pos[lo, :2]) < 15.0:
                hi, lo = int(rng.choice(self.high)), int(rng.choice(self.low))
            i0, i1 = (lo, hi) if kind == "out_in" else (hi, lo)
        else:
            pool = self.high if kind == "behind" and len(self.high) >= 3 else np.arange(self.n)   # (one level: both t and s negative)
            i0, i1 = [int(v) for v in rng.choice(pool, 2, replace=False)]
            while np.linalg.norm(pos[i0, :2] - pos[i1, :2]) < 15.0:   # (not the pair 1.5 m apart, nor a baseline that makes kappa large)
                i0, i1 = [int(v) for v in rng.choice(pool, 2, replace=False)]
        if kind == "behind":
            b = (pos[i1] - pos[i0]) * [1, 1, 0]
            b /= np.linalg.norm(b)
            g0, g1 = pos[i0] * [1, 1, 0] - 40 * b, pos[i1] * [1, 1, 0] + 40 * b
            return [i0, i1], [self.proj(g0, i0) + rng.normal(0, 3, 2), self.proj(g1, i1) + rng.normal(0, 3, 2)], P
        if kind == "behind_one":
            b = (pos[i1] - pos[i0]) * [1, 1, 0]
            b /= np.linalg.norm(b)
            g0, g1 = pos[i0] * [1, 1, 0], pos[i1] * [1, 1, 0] + 40 * b
            return [i0, i1], [self.proj(g0, i0) + rng.normal(0, 3, 2), self.proj(g1, i1) + rng.normal(0, 3, 2)], P
        px = [self.proj(P, i0) + rng.normal(0, 0.3, 2), self.proj(P, i1) + rng.normal(0, 0.3, 2)]
        if kind in ("in_out", "out_in"):
            hi, lo = (i0, i1) if kind == "in_out" else (i1, i0)
            gap = 2 * 5.0 * (pos[hi, 2] - P[2]) / F
            k = 1 if kind == "in_out" else 0
            px[k] = px[k] + self._epipolar_normal(lo, hi, P) * gap * F / (pos[lo, 2] - P[2])
        elif kind == "out_out":      # a gap that is 12 px in a camera 140 m up, 24 px in one 70 m up
            px[1] = px[1] + self._epipolar_normal(i1, i0, P) * 2 * 12.0 * HIGH / (pos[i1, 2] - P[2])
        return [i0, i1], px, P

    def track(self, name, family, n, first="in_in", inliers="all", edge=False, extra=None, pair=None, P=None, apart=None):
        """a track of n members.  inliers: "all", or the members from 2 on that observe the first pair's point with 0.3 px of
        noise - the others sit 30 to 150 px off.  edge: the members from 2 on alternate between 7.99 px (in) and 8.01 px (out).
        extra: {member: (image, pixel) or callable(M) -> (image, pixel)} placed by the caller.  apart: {member: earlier member}
        that must not share an image (a pair from one image has equal origins and t = s = 0)"""
        rng = self.rng
        images, px, P = self.first_pair(first, pair, P)
        ref = eval_track(self.cams, np.array(images), np.array(px), LD, self.i3d)
        M = ref["first"]["point"].astype(np.float64) if ref["first"]["ok"] else P
        rest = self.images_for(n - 2)
        for k in range(2, n):
            if extra and k in extra:
                img, p = extra[k](M) if callable(extra[k]) else extra[k]
            else:
                img = rest[k - 2]
                if apart and k in apart and images[apart[k]] == img:
                    img = (img + 1) % self.n
                u = rng.normal(0, 1, 2)
                u /= np.linalg.norm(u)
                if edge:
                    p = self.proj(M, img) + u * (7.99 if k % 2 == 0 else 8.01)
                elif inliers == "all" or k in inliers:
                    p = self.proj(M, img) + rng.normal(0, 0.3, 2)
                else:
                    p = self.proj(M, img) + u * rng.uniform(30, 150)
            images.append(int(img)), px.append(np.asarray(p, np.float64))
        return dict(name=name, family=family, images=np.array(images, np.int64), px=np.ascontiguousarray(np.array(px), np.float64))


def _finish_scene(name, cams, tracks, image_to_3d, calls=None):
    """the reference of every track, the margins, the index's features and the tracks' members"""
    kept, dropped = [], []
    for t in tracks:
        t["ref"] = eval_track(cams, t["images"], t["px"], LD, image_to_3d)
        t["why"] = margin_reasons(cams, t["images"], t["ref"])
        (dropped if t["why"] else kept).append(t)
    per_image = [[] for _ in range(cams["n"])]
    for t in kept:
        t["local"] = []
        for img, p in zip(t["images"], t["px"]):
            t["local"].append(len(per_image[img]))
            per_image[img].append(p)
    off = np.concatenate([[0], np.cumsum([len(f) for f in per_image])])
    for t in kept:
        t["members"] = np.array([off[i] + k for i, k in zip(t["images"], t["local"])], np.uint32)
    desc = synth.descriptors_for_ids(np.arange(off[-1], dtype=np.int64) + 7000000)
    features = [(np.array(f, np.float64).reshape(-1, 2), desc[off[i]:off[i + 1]]) for i, f in enumerate(per_image)]
    return dict(name=name, cams=cams, tracks=kept, dropped=dropped, generated=len(tracks), features=features, total=int(off[-1]),
                feat_off=off)


def _general_tracks(mk, tag, rich):
    """the families on one set of cameras.  rich: every family in full (the 30-image scene); otherwise one of each"""
    T, reps = [], (2 if rich else 1)
    for n in TRACK_SIZES:
        for k in range(reps):
            T.append(mk.track("%s/size_n%d_all_k%d" % (tag, n, k), "sizes", n))
            if n >= 3:
                some = set(int(v) for v in mk.rng.choice(np.arange(2, n), max(1, (n - 2) * 4 // 5), replace=False)) if n > 3 else set()
                T.append(mk.track("%s/size_n%d_outliers_k%d" % (tag, n, k), "sizes", n, inliers=some))
    pair_kind = {(0, 1): "in_in", (0, 2): "in_out", (1, 2): "out_in", (5, 6): "out_out"}
    for a, b in SECOND_PAIRS:
        for n in (8, 40):
            for k in range(reps):
                inl = {i for i in range(2, n) if i >= max(b, 2) and (i <= b + 1 or i % 3 == 0)} | ({a} if a >= 2 else set())
                T.append(mk.track("%s/second_%d_%d_n%d_k%d" % (tag, a, b, n, k), "second", n, first=pair_kind[(a, b)], inliers=inl,
                                  apart={b: a} if b >= 2 else None))
    for a, b in LANE_PAIRS:
        for k in range(reps):
            T.append(mk.track("%s/second_%d_%d_n140_k%d" % (tag, a, b, k), "lanes", 140, first="out_out", inliers={a, b, b + 1, 133, 134}, apart={b: a}))
    for n in (5, 40):
        for count in (0, 1):
            T.append(mk.track("%s/few_inliers_n%d_%d" % (tag, n, count), "few", n, first="out_out", inliers={3} if count else set()))
    for n in (2, 3, 40):
        T.append(mk.track("%s/behind_n%d" % (tag, n), "behind", n, first="behind"))
        T.append(mk.track("%s/behind_one_n%d" % (tag, n), "behind", n, first="behind_one"))
    for n in (8, 40):
        T.append(mk.track("%s/edge_n%d" % (tag, n), "edge", n, first="out_out", edge=True, apart={3: 2, 4: 2}))
    if mk.n >= 3:       # the second pair fails: the two cameras 1.5 m apart look past the point on either side, within 8 px of it
        cams = mk.cams
        b = cams["pos"][mk.n - 1] - cams["pos"][0]
        b /= np.linalg.norm(b)
        for n in (6, 40):
            extra = {2: lambda M: (0, mk.proj(M - 0.9 * b, 0)), 3: lambda M: (mk.n - 1, mk.proj(M + 0.9 * b, mk.n - 1))}
            T.append(mk.track("%s/second_pair_behind_n%d" % (tag, n), "second_fails", n, first="out_out", inliers={2, 3, n - 1}, extra=extra))
    for k in range(110 if rich else 24):
        n = int(mk.rng.integers(2, 7))
        inl = set(int(v) for v in np.arange(2, n)[mk.rng.uniform(size=n - 2) < 0.7])
        T.append(mk.track("%s/bulk%d" % (tag, k), "bulk", n, inliers=inl))
    order = mk.rng.permutation(len(T))
    return [T[i] for i in order]


def _exact_tracks(image_to_3d):
    """identity-oriented, undistorted cameras with integer geometry: directions that are equal or opposite bit for bit"""
    pos = np.array([[0, 0, 64], [2, 0, 64], [0, 0, 32], [64, 0, 64], [-64, 0, 64], [40, 24, 64]], np.float64)
    q = np.array([Q_DOWN, Q_DOWN, Q_IDENTITY, Q_DOWN, Q_DOWN, Q_DOWN])
    cams = dict(pos=pos, q=q, models=np.tile(EXACT_MODEL, (6, 1)), n=6)
    mk = _TrackMaker(cams, 5600, image_to_3d, focal=EXACT_MODEL[0])
    rng, T = mk.rng, []

    def manual(name, family, members):
        T.append(dict(name="exact/" + name, family=family, images=np.array([m[0] for m in members], np.int64),
                      px=np.ascontiguousarray([m[1] for m in members], np.float64)))

    filler = lambda k: [(int(rng.integers(3, 6)), rng.uniform([100, 100], [900, 700])) for _ in range(k)]
    for k, p in enumerate(([300.0, 200.0], [512.0, 384.0], [733.5, 100.25])):
        manual("equal_n2_%d" % k, "equal", [(0, p), (1, p)])
        manual("equal_n40_%d" % k, "equal", [(0, p), (1, p)] + filler(38))
    for k, (d, y) in enumerate(((100.0, 384.0), (37.5, 500.0), (0.0, 384.0))):
        manual("opposite_n2_%d" % k, "opposite", [(0, [512.0 - d, y]), (2, [512.0 + d, y])])
        manual("opposite_n40_%d" % k, "opposite", [(0, [512.0 - d, y]), (2, [512.0 + d, y])] + filler(38))

    def off_image(k, M):
        img = 3 + k % 3
        return img, mk.proj(M, img) + [60.0, 45.0]

    # the second pair's directions are equal: cameras 0 and 1, 2 m apart, see a point 128 m below them 8 px apart, and one
    # pixel half way is an inlier of both
    for n in (5, 40):
        half = lambda M: 0.5 * (mk.proj(M, 0) + mk.proj(M, 1))
        extra = {2: lambda M: (0, half(M)), 3: lambda M: (1, half(M))}
        extra.update({k: (lambda M, k=k: off_image(k, M)) for k in range(4, n)})
        T.append(mk.track("exact/second_pair_equal_n%d" % n, "second_fails", n, first="out_out", extra=extra, pair=(3, 5),
                          P=[rng.uniform(-5, 10), rng.uniform(-5, 10), rng.uniform(-70, -58)]))
    # the clamp: camera 2 looks up from above the point, which is behind it; the member's pixel is where the point would be
    # without the clamp.  (The first pair's rays are at right angles - kappa = 1 - so that the point's bound times the clamped
    # member's f / 1e-3 stays inside the sensitivity margin.)
    for n in (6, 40):
        extra = {2: lambda M: (2, mk.proj(M, 2, clamp=False))}
        extra.update({3: lambda M: (5, mk.proj(M, 5) + [0.2, -0.1]), 4: lambda M: (3, mk.proj(M, 3) + [-0.3, 0.15])})
        extra.update({k: (lambda M, k=k: off_image(k, M)) for k in range(5, n)})
        T.append(mk.track("exact/behind_camera_n%d" % n, "clamp", n, first="out_out", extra=extra, pair=(3, 4),
                          P=[rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-2, 2)]))
    return cams, T


_TRI = {}


def tri_scenes(image_to_3d):
    """the scenes of the triangulation tests; image_to_3d: the oracle's (pixels [k][2], model10) -> rays [k][3]"""
    if "scenes" in _TRI:
        return _TRI["scenes"]
    out = []
    for n, dists, seed in ((2, (None,), 5200), (3, (None, DIST_A, DIST_B), 5300), (30, (None, DIST_A, DIST_B), 5400)):
        cams = _tri_cameras(np.random.default_rng(seed), n, dists)
        mk = _TrackMaker(cams, seed + 1, image_to_3d)
        out.append(_finish_scene("tri%d" % n, cams, _general_tracks(mk, "tri%d" % n, rich=n == 30), image_to_3d))
    cams, T = _exact_tracks(image_to_3d)
    out.append(_finish_scene("exact", cams, T, image_to_3d))
    for s in out:
        s["calls"] = _calls(s)
    _TRI["scenes"] = out
    return out


def _calls(s):
    """the triangulate calls of a scene: name -> track numbers.  Every scene: all tracks.  The 30-image scene also the counts
    around the thread kernel's workgroup of 128 and the wavefront kernel's four tracks per workgroup"""
    T = s["tracks"]
    large = [i for i, t in enumerate(T) if len(t["images"]) > TRI_LARGE]
    small = [i for i, t in enumerate(T) if len(t["images"]) <= TRI_LARGE]
    calls = {"all": list(range(len(T))), "empty": []}
    if s["name"] == "tri30":
        calls.update({"one": small[:1], "one_large": large[:1], "first127": list(range(127)), "first128": list(range(128)),
                      "first129": list(range(129)), "large4": small[:9] + large[1:5] + small[9:12],
                      "large5": large[5:8] + small[20:30] + large[8:10], "large_only": large})
    return calls


def call_arrays(s, track_numbers):
    """(track_start [k + 1], track_member) of a call"""
    T = [s["tracks"][i] for i in track_numbers]
    start = np.concatenate([[0], np.cumsum([len(t["members"]) for t in T])]).astype(np.uint32)
    member = np.concatenate([t["members"] for t in T]).astype(np.uint32) if T else np.zeros(0, np.uint32)
    return np.ascontiguousarray(start), np.ascontiguousarray(member)


def tri_fp64(s, t, image_to_3d, mutation=None):
    """the kernels restated in fp64 on one track"""
    assert mutation is None or mutation in TRI_MUTATIONS + EQUIVALENT_MUTATIONS, mutation
    return eval_track(s["cams"], t["images"], t["px"], np.float64, image_to_3d, mutation)


def check_track(t, valid, point, C=C_TRI):
    """a result (valid, point [3] fp64) against the track's reference: (problem or None, error / bound at C = 1 or None)"""
    ref = t["ref"]
    if bool(valid) != ref["valid"]:
        return "%s: valid %d, reference %d" % (t["name"], bool(valid), ref["valid"]), None
    if not ref["valid"]:
        return None, None
    b, kappa, scale = point_bound(ref, 1.0)
    err = float(np.max(np.abs(np.asarray(point, np.float64).astype(LD) - ref["point"])))
    ratio = err / b
    if not ratio <= C:
        return "%s: error %.3g = %.3g x 2^-53 kappa scale (kappa %.3g, scale %.3g), C_TRI = %g" % (t["name"], err, ratio, kappa, scale, C), ratio
    return None, ratio


def tri_facts(s):
    """what a triangulation scene contains, from the reference"""
    f = dict(tracks=len(s["tracks"]), generated=s["generated"], dropped=[(t["name"], t["why"]) for t in s["dropped"]], families={},
             sizes=set(), pairs_small=set(), pairs_large=set(), valid=0, first_fails=0, second_fails=0, few=0, denom_zero=0,
             behind_both=0, behind_one=0, repeated_image_in_large=0, distorted_pairs=0)
    for t in s["tracks"]:
        r, n = t["ref"], len(t["images"])
        f["families"][t["family"]] = f["families"].get(t["family"], 0) + 1
        f["sizes"].add(n)
        f["valid"] += r["valid"]
        if r["valid"] and r["second"] is not None:
            (f["pairs_large"] if n > TRI_LARGE else f["pairs_small"]).add(r["pair"])
        if r["valid"] and s["cams"]["models"][t["images"][list(r["pair"])], 3:8].any():
            f["distorted_pairs"] += 1
        for I in (r["first"], r["second"]):
            if I is None or I["ok"]:
                continue
            f["denom_zero"] += bool(I["denom"] == 0)
            if I["computed"]:
                f["behind_both"] += bool(I["t"] < 0 and I["s"] < 0)
                f["behind_one"] += bool((I["t"] < 0) != (I["s"] < 0))
        f["first_fails"] += not r["first"]["ok"]
        f["second_fails"] += bool(r["second"] is not None and not r["second"]["ok"])
        f["few"] += bool(r["first"]["ok"] and r["inliers"].sum() < 2)
        if n > 64:
            f["repeated_image_in_large"] += bool(len(set(t["images"].tolist())) < n)
    return f

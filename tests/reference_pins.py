"""Cases of tests/golden/reference_pins.npz (written by scripts/make_reference_pins.py): the answers of the reference's own
std-only headers (jk::tree::KDTree, GridFilter, UnionFind, KMeans, hilbert.hpp, interleave.hpp, ankerl::unordered_dense),
compiled through oracle/ref_shim.cpp into oracle/_ref/libref.so, on the seeded inputs below.  The tests check the
restatement against these stored answers, so they need neither the reference's sources nor the library that is built from
them.  Every generator yields (key, inputs) in a fixed order; the recorder and the tests walk the same generators."""
import ctypes as C
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_pins.npz")
_CACHE = None


def golden():
    """{key: array} of the stored reference answers."""
    global _CACHE
    if _CACHE is None:
        with np.load(GOLDEN) as z:
            _CACHE = {k: z[k] for k in z.files}
    return _CACHE


# ---- inputs --------------------------------------------------------------------------------------------------------------
def hilbert_cases():
    rng = np.random.default_rng(0)
    for order in (2, 8, 1024, 4096):
        yield f"hilbert/{order}", (order, rng.integers(0, order, (200, 2)))


def kdtree_cases():
    """(cams, knn queries), (pts, ball queries): the 11 nearest cameras of a point and the features in a 150 px disc."""
    rng = np.random.default_rng(3)
    cams = rng.uniform(0, 500, (300, 3)) * [1, 1, 0.02] + [0, 0, 100]
    knn_q = [rng.uniform(-50, 550, 3) * [1, 1, 0] for _ in range(50)]
    pts = rng.uniform(0, 1000, (2000, 2))
    pts[7] = [400.0, 300.0 + 150.0]                      # exactly on the circle: outside (`<`)
    ball_q = [np.array([400.0, 300.0])] + [rng.uniform(0, 1000, 2) for _ in range(30)]
    return cams, knn_q, pts, ball_q


def subsample_cases(synth):
    rng = np.random.default_rng(11)
    for i, (n, spacing) in enumerate(((1, 40.0), (50, 40.0), (4000, 40.0), (4000, 8.0), (2000, 123.5))):
        loc = rng.uniform(0, 4000, (n, 2))
        # heavy strength ties exercise the unstable std::sort path both sides share
        strength = (rng.integers(0, 50, n) / 50).astype(np.float32)
        yield f"subsample/{i}", (loc, strength, spacing)
    g = synth.make_grid(1, 2, feats=1024, seed=5)
    loc, st, _, _ = g.image(0)
    yield "subsample/grid", (loc, st, 40.0)


def knn_grid(synth):
    return synth.make_grid(4, 6, feats=64, seed=1).position[:, :2]


def grid_filter_cases():
    for res in (0.15, 0.1, 0.05, 0.075):
        rng = np.random.default_rng(int(res * 1000))
        for trial in range(20):
            n = int(rng.integers(1, 800))
            xy = np.ascontiguousarray(rng.uniform(-0.05, 1.05, (n, 2)))  # includes cells left of / above the image
            score = np.ascontiguousarray(np.round(rng.uniform(0, 1, n), 2 if trial % 2 else 12))  # with and without ties
            value = np.ascontiguousarray(np.arange(n, dtype=np.uint64))
            yield f"grid_filter/{res}/{trial}/distinct", (xy, score, value, res)
            # values that repeat (a track root entered once per image cell): the set semantics of _best
            value = np.ascontiguousarray(rng.integers(0, max(2, n // 3), n).astype(np.uint64))
            yield f"grid_filter/{res}/{trial}/repeated", (xy, score, value, res)


GRID_CELL_KEYS = [(0, 0), (3, 9), (-1, 2), (2, -1), (-1, -1), (2 ** 20, 5)]


def union_find_cases():
    rng = np.random.default_rng(4)
    for trial in range(30):
        n = int(rng.integers(2, 2000))
        pairs = np.ascontiguousarray(rng.integers(0, n, (int(rng.integers(1, 2 * n)), 2)).astype(np.uint64))
        yield f"union_find/{trial}", (n, pairs)


def kmeans_cases():
    rng = np.random.default_rng(11)
    for trial in range(12):
        n, k = int(rng.integers(20, 600)), int(rng.integers(2, 9))
        pts = rng.normal(size=(n, 3)) * rng.uniform(0.5, 20, 3)
        if trial % 3 == 0:   # clumps: small clusters get re-seeded next to big ones (KMeans.hpp:196-214)
            pts[: n // 2] = pts[: n // 2] * 0.01 + 50
        for iters in (1, 2, 5, 11):
            yield f"kmeans/{trial}/{iters}", (pts, k, iters)


def dense_set_cases():
    """Insert / erase sequences (erase of k encoded as -k - 1) and the order a vector with swap-and-pop would hold."""
    rng = np.random.default_rng(1)
    for trial in range(20):
        ops, model, live = [], [], set()
        for step in range(200):
            if live and rng.uniform() < 0.35:
                k = int(rng.choice(sorted(live)))
                ops.append(-k - 1)
                i = model.index(k)
                model[i] = model[-1]
                model.pop()
                live.discard(k)
            else:
                k = int(rng.integers(0, 1 << 40))
                if k in live:
                    continue
                ops.append(k)
                model.append(k)
                live.add(k)
        yield f"dense_set/{trial}", (np.array(ops, np.int64), model)


INTERLEAVE_LISTS = (np.arange(0, 4, dtype=np.uint64), np.arange(10, 16, dtype=np.uint64), np.array([20], np.uint64))
# test_tree.cpp:10-38: (1, 2), (1, 3), (7, 7) and the monster at (6, 6) as a fourth point
KDTREE_KNOWN_POINTS = np.array([[1, 2], [1, 3], [7, 7], [6, 6]], np.float64)


# ---- the recorder (needs oracle/_ref/libref.so) ------------------------------------------------------------------------
def record(pyoracle, synth):
    """Every stored answer, computed by the reference's headers through oracle/_ref/libref.so."""
    r = pyoracle.ref()
    if r is None:
        raise RuntimeError("oracle/_ref/libref.so is not built (make -C oracle ref, with the reference's sources at hand)")
    u64p, f64p = pyoracle.u64p, pyoracle.f64p
    out = {}
    r.ref_hilbert_xy2d.restype = C.c_uint32
    for key, (order, xy) in hilbert_cases():
        out[key] = np.array([r.ref_hilbert_xy2d(int(order), int(x), int(y)) for x, y in xy], np.uint64)
    r.ref_knn3.restype = C.c_size_t
    r.ref_knn3.argtypes = [f64p, C.c_size_t, f64p, C.c_size_t, u64p]
    r.ref_ball2.restype = C.c_size_t
    r.ref_ball2.argtypes = [f64p, C.c_size_t, f64p, C.c_double, u64p]
    cams, knn_q, pts, ball_q = kdtree_cases()
    buf = np.zeros(len(pts), np.uint64)
    for i, q in enumerate(knn_q):
        k = r.ref_knn3(cams, len(cams), np.ascontiguousarray(q), 11, buf)
        out[f"knn3/{i}"] = buf[:k].copy()
    for i, q in enumerate(ball_q):
        k = r.ref_ball2(pts, len(pts), np.ascontiguousarray(q), 150.0 ** 2, buf)
        out[f"ball2/{i}"] = buf[:k].copy()
    for key, (loc, st, spacing) in subsample_cases(synth):
        out[key] = pyoracle.ref_subsample(loc, st, spacing)
    out["knn_grid"] = pyoracle.ref_knn(knn_grid(synth), 10)
    r.ref_grid_filter_values.argtypes = [f64p, f64p, u64p, C.c_size_t, C.c_double, u64p, C.c_void_p]
    for key, (xy, score, value, res) in grid_filter_cases():
        best, n = np.zeros(len(value) + 1, np.uint64), C.c_size_t(0)
        r.ref_grid_filter_values(xy, score, value, len(value), res, best, C.addressof(n))
        out[key] = np.array(sorted(set(best[:n.value].tolist())), np.uint64)
    r.ref_grid_cell_key.restype = C.c_uint64
    r.ref_grid_cell_key.argtypes = [C.c_int, C.c_int]
    out["grid_cell_key"] = np.array([r.ref_grid_cell_key(i, j) for i, j in GRID_CELL_KEYS], np.uint64)
    r.ref_union_find.argtypes = [C.c_size_t, u64p, C.c_size_t, u64p]
    for key, (n, pairs) in union_find_cases():
        roots = np.zeros(n, np.uint64)
        r.ref_union_find(n, pairs, len(pairs), roots)
        out[key] = roots
    for key, (pts3, k, iters) in kmeans_cases():
        a, c, s = pyoracle.kmeans3(pts3, k, iters, use_ref=True)
        out[key + "/assignment"], out[key + "/centroids"], out[key + "/sizes"] = a, c, s
    r.ref_dense_set_order.restype = C.c_size_t
    r.ref_dense_set_order.argtypes = [np.ctypeslib.ndpointer(np.int64), C.c_size_t, u64p]
    for key, (ops, _) in dense_set_cases():
        order = np.zeros(len(ops) + 1, np.uint64)
        n = r.ref_dense_set_order(ops, len(ops), order)
        out[key] = order[:n].copy()
    r.ref_interleave3.restype = C.c_size_t
    r.ref_interleave3.argtypes = [u64p, C.c_size_t, u64p, C.c_size_t, u64p, C.c_size_t, C.c_int, u64p]
    a, b, c = INTERLEAVE_LISTS
    order = np.zeros(16, np.uint64)
    n = r.ref_interleave3(a, len(a), b, len(b), c, len(c), 1, order)      # (full_dispersal = true, the test's default)
    out["interleave3"] = order[:n].copy()
    out["interleave3_empty"] = np.array([r.ref_interleave3(a, 0, b, 0, c, 0, 1, order)], np.uint64)
    knn = np.zeros((4, 3), np.uint64)
    r.ref_knn(np.ascontiguousarray(KDTREE_KNOWN_POINTS), 4, 3, knn)
    out["kdtree_known"] = knn
    return out

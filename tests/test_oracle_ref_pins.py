"""Pins restated building blocks against the reference's OWN code: the answers of its std-only headers
include/opencalibration/relax/grid_filter.hpp (+ external/unordered_dense), types/union_find.hpp and geometry/KMeans.hpp
on seeded inputs, stored in tests/golden/reference_pins.npz (tests/reference_pins.py, scripts/make_reference_pins.py).
These are the pieces of a14 (grid filter of the inliers) and a15 (union-find tracks, per-cell longest-track filter) that
decide WHICH residual blocks a relax problem gets."""
import ctypes as C

import numpy as np
import pytest

import reference_pins as rp


@pytest.fixture(scope="module")
def ocx(oracle):
    L = oracle.lib()
    u64p, f64p = oracle.u64p, oracle.f64p
    L.ocx_grid_filter_values.argtypes = [f64p, f64p, u64p, C.c_size_t, C.c_double, u64p, C.c_void_p]
    L.ocx_union_find.argtypes = [C.c_size_t, u64p, C.c_size_t, u64p]
    L.ocx_grid_cell_key.restype = C.c_uint64
    L.ocx_grid_cell_key.argtypes = [C.c_int, C.c_int]
    return L


def _filter(lib, xy, score, value, res):
    out, n = np.zeros(len(value) + 1, np.uint64), C.c_size_t(0)
    lib.ocx_grid_filter_values(xy, score, value, len(value), res, out, C.addressof(n))
    return set(out[:n.value].tolist())


@pytest.mark.parametrize("res", [0.15, 0.1, 0.05, 0.075])
def test_grid_filter_matches_reference_header(ocx, res):
    gold = rp.golden()
    cases = [c for c in rp.grid_filter_cases() if c[1][3] == res]
    assert len(cases) == 40
    for key, (xy, score, value, r) in cases:
        assert _filter(ocx, xy, score, value, r) == set(gold[key].tolist()), key


def test_grid_cell_key_matches_reference_header(ocx):
    got = [ocx.ocx_grid_cell_key(i, j) for i, j in rp.GRID_CELL_KEYS]
    assert got == rp.golden()["grid_cell_key"].tolist()


def test_union_find_matches_reference_header(ocx):
    gold = rp.golden()
    for key, (n, pairs) in rp.union_find_cases():
        b = np.zeros(n, np.uint64)
        ocx.ocx_union_find(n, pairs, len(pairs), b)
        assert np.array_equal(gold[key], b), key  # the same ROOT ids, not just the same partition: track order follows the roots


def test_kmeans_matches_reference_header(oracle):
    """include/opencalibration/geometry/KMeans.hpp against the restatement used by the partitioning of the relax stage: same
    clusters (sizes, centroids bit for bit, assignment), after 0..10 iterate() calls."""
    gold = rp.golden()
    for key, (pts, k, iters) in rp.kmeans_cases():
        a2, c2, s2 = oracle.kmeans3(pts, k, iters, use_ref=False)
        assert (np.array_equal(gold[key + "/sizes"], s2) and np.array_equal(gold[key + "/centroids"], c2)
                and np.array_equal(gold[key + "/assignment"], a2)), key

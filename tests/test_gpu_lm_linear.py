"""The linear algebra of one LM step on the device (ochip_debug_lm_step: lm_build_kernel, chol_tiles_kernel or the launch
chain, back_solve_kernel / back_solve_regions_kernel, as lm_solve launches them) against a plain fp64 / longdouble
reference (tests/lm_fixtures.py): W bit for bit, the factor, the forward and backward solves and the model cost change
within componentwise bounds, failure flags, repeatability of the dynamically claimed tile factorisation, and the plan's
claim order.  The resident chain's factorisations (relax_chain.hip: phase_chol and the one-thread Cholesky of small systems) are
held to the same bounds through the chain's trace seam by tests/test_gpu_chain_trace.py.  Not covered here: the Schur
elimination of the 3-D points (relax_points.hip)."""
import json

import numpy as np
import pytest

import lm_fixtures as F
from opencalibration_amd import capi

pytestmark = pytest.mark.gpu

ROUTES = (0, 1)        # tiles, launch chain
BACKS = (1, 2, 3)      # single workgroup, regions with x in LDS, regions with x in HBM
RATIOS = {}            # assertion family -> (largest ratio of error to bound, case)


def _note(family, ratio, case):
    if family not in RATIOS or ratio > RATIOS[family][0]:
        RATIOS[family] = (float(ratio), case.name)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nLM_LINEAR_RATIOS " + json.dumps({k: [round(v[0], 4), v[1]] for k, v in sorted(RATIOS.items())}))


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def slots(ctx):
    r = ctx.debug_lm_step(np.eye(3), np.ones(3), np.ones(3), np.ones(3), 1.0, [3], 3)
    assert r["slots"] > 0
    return r["slots"]


def _run(ctx, c, route, back, want=True):
    return ctx.debug_lm_step(c.A, c.g, c.scale, c.diagonal, c.radius, c.env_end, c.tail_begin, c.region_begin, route=route,
                             back=back, want_L=want, want_W=want)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _profile(A):
    """(i, j), j <= i, at or right of the first non-zero of row i of A: the exact factor's profile (no fill left of it)"""
    n = len(A)
    nz = (np.tril(A) != 0) | np.eye(n, dtype=bool)
    first = np.argmax(nz, axis=1)
    j = np.arange(n)
    return (j[None, :] >= first[:, None]) & np.tri(n, dtype=bool)


def _check_solution(c, Wa, r, route, back):
    """the step's backward error and the model cost change of a result with fail = 0"""
    n = c.n
    x = r["x"]
    assert np.all(np.isfinite(x)), (c.name, route, back)
    bw = F.backward_ratio(Wa, x)
    _note("backward |Wx-gs|", bw, c)
    assert bw <= 1.0, (c.name, route, back, bw)
    mr = F.model_ratio(c, x, r["scal1"])
    _note("model cost change", mr, c)
    assert mr <= 1.0, (c.name, route, back, r["scal1"], F.model_change(c, x))
    if c.well and n <= 1024:
        fe = F.forward_error_ratio(Wa, x, c.ref["x"])
        _note("forward error vs cho_solve", fe, c)
        assert fe <= 1.0, (c.name, route, back, fe)


def check_case(ctx, slots, c):
    n = c.n
    Wa = F.reference_W(c)
    expect_plan = F.plan(n, c.env_end, c.tail_begin, c.region_begin, slots=slots)
    results = {}
    for route in ROUTES:
        a = _run(ctx, c, route, 0)
        b = _run(ctx, c, route, 0)
        results[route] = a
        # the plan: stored tiles, regions and the claim order as lm_system_resize is documented to choose them
        assert (a["tiles"], a["regions"], a["order"]) == (expect_plan["n_tiles"], expect_plan["regions"], expect_plan["order"]), \
            (c.name, a["tiles"], a["regions"], a["order"], expect_plan["n_tiles"], expect_plan["regions"], expect_plan["order"])
        assert a["back"] == 2  # what lm_solve runs: the regions' kernel (one region for a single band), x in LDS
        # W as built: a few IEEE products in a fixed order (-ffp-contract=off), bit for bit
        same = (_bits(a["W"]) == _bits(Wa)) | (np.isnan(a["W"]) & np.isnan(Wa))
        assert same.all(), (c.name, route, np.argwhere(~same)[:5])
        # repeatable: the tiles are claimed dynamically but each is computed once, in a fixed order
        for k in ("x", "y", "L"):
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (c.name, route, k)
        assert _bits(np.float64(a["scal1"])) == _bits(np.float64(b["scal1"])) and a["fail"] == b["fail"]
        if c.expect == "fail":
            assert a["fail"] == 1, (c.name, route)
            continue
        if c.expect == "nan_g":
            assert a["fail"] == 1 or not np.isfinite(a["scal1"]), (c.name, route, a["fail"], a["scal1"])
            continue
        assert a["fail"] == 0, (c.name, route)
        L, y = a["L"], a["y"]
        # the factor: exactly 0 outside the profile (and so outside the envelope), Higham's componentwise bound inside
        assert not ((L != 0) & ~_profile(c.A)).any(), (c.name, route)
        assert np.all(np.isfinite(L)) and np.all(np.isfinite(y))
        fr = F.factor_ratio(Wa, L, c.plan["stored"])
        _note("factor |W-LL'|", fr, c)
        assert fr <= 1.0, (c.name, route, fr)
        fw = F.forward_ratio(L, y, Wa[n])
        _note("forward |Ly-gs|", fw, c)
        assert fw <= 1.0, (c.name, route, fw)
        _check_solution(c, Wa, a, route, 0)
        xs = {}
        for back in BACKS:
            r = _run(ctx, c, route, back, want=False)
            assert r["back"] == back and r["fail"] == 0
            assert np.array_equal(_bits(r["y"]), _bits(y)), (c.name, route, back)  # the same factorisation
            _check_solution(c, Wa, r, route, back)
            xs[back] = r
        # x in LDS or in HBM: the same arithmetic, the same bits; lm_solve's choice is the LDS one
        assert np.array_equal(_bits(xs[2]["x"]), _bits(xs[3]["x"])) and np.array_equal(_bits(xs[2]["x"]), _bits(a["x"]))
    return results


@pytest.mark.parametrize("case", F.all_cases(), ids=str)
def test_lm_step_against_fp64(ctx, slots, case):
    check_case(ctx, slots, case)


def test_cameras_1000(ctx, slots):
    """n = 3003 in two regions with a dense tail of 3: the size of the 1 000-camera relax"""
    c = F.big_case()
    res = check_case(ctx, slots, c)
    assert res[0]["order"] == 2 and res[0]["regions"] == 2


def test_column_order(ctx, slots):
    """a dense tail large against the device (tail tiles * 8 > slots): plain column order"""
    c = F.column_order_case(slots)
    res = check_case(ctx, slots, c)
    assert res[0]["order"] == 0


@pytest.mark.parametrize("rows,cols,mesh", F.REAL_SCENES)
def test_real_relax_system(ctx, slots, rows, cols, mesh):
    """J'J and J'r of a mesh relax problem as the general engine evaluates them now (a 2 x 2 mesh: the heights are the
    dense tail; 3 x 3: they join the cameras in the band), with the envelope derived from the non-zero pattern"""
    cost, JtJ, Jtr, order = ctx.relaxg_evaluate(F.mesh_scene(rows, cols, seed=rows * cols, mesh=mesh))
    n_cams = rows * cols
    assert np.isfinite(cost) and cost > 0 and len(Jtr) >= 3 * n_cams + mesh * mesh and np.any(Jtr != 0)
    assert np.array_equal(JtJ, JtJ.T)
    c = F.real_case(f"mesh_{rows}x{cols}_{mesh}", JtJ, Jtr, order, n_cams, mesh * mesh)
    assert (c.tail_begin < c.n) == (mesh * mesh <= 8)
    check_case(ctx, slots, c)


def test_every_claim_order_is_reached(slots):
    """regions, tail first and plain column order each have a case on this device (check_case asserts the seam's report)"""
    cases = F.all_cases() + [F.big_case(), F.column_order_case(slots)]
    assert {F.plan(c.n, c.env_end, c.tail_begin, c.region_begin, slots=slots)["order"] for c in cases} == {0, 1, 2}


def test_empty_system(ctx):
    r = ctx.debug_lm_step(np.zeros((0, 0)), [], [], [], 1.0, [], 0)
    assert r["fail"] == 0 and r["scal1"] == 0.0 and len(r["x"]) == 0


def test_envelope_violation_is_refused(ctx):
    A = np.eye(130)
    A[100, 0] = A[0, 100] = 0.5  # row block 1 of column block 0: neither band (env_end 64) nor tail (the last block)
    with pytest.raises(capi.OchipError):
        ctx.debug_lm_step(A, np.ones(130), np.ones(130), np.ones(130), 1.0, F.band_env(130, 0), 130)

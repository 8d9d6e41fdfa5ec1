"""The colour-balance solve on the CPU route (csrc/host/color_balance.cpp, csrc/color_balance.hpp), without a device:

1. the reference's unit tests restated (test/test_color_balance.cpp): the functors' known answers through the evaluation
   seam, and its four solves with its own tolerances;
2. the CPU route against the oracle's Ceres restatement (oracle/mini_ceres.hpp) driven by
   tests/color_balance_oracle_driver.cpp, live and as recorded under tests/golden/color_balance/: equal iteration counts
   and success, parameters within 1e-6, final cost within 1e-9 relative - on scenes none of whose termination decisions
   sits within a factor 4 of its threshold (asserted on the yardstick alone).  No scene that stops at the 20-iteration
   limit is among them: the slowly converging scenes tried (offsets of 300 - 3 000 Lab units) creep through the function
   tolerance and fail that condition;
3. the gauge removal against numpy.linalg.lstsq;
4. the evaluation seam against a long-double restatement, within c u normwise bounds."""
import json
import os

import numpy as np
import pytest

import color_balance_fixtures as F
from opencalibration_amd import capi, host


def _one(lab_a, lab_b, cams=(1, 2), models=(7, 7), r=(0, 0), th=(0, 0), a_xy=(0, 0), b_xy=(0, 0), n=1):
    c = F.make_corr(n)
    c["lab_a"], c["lab_b"] = lab_a, lab_b
    c["camera_id_a"], c["camera_id_b"] = cams
    c["model_id_a"], c["model_id_b"] = models
    c["normalized_radius_a"], c["normalized_radius_b"] = r
    c["view_angle_a"], c["view_angle_b"] = th
    c["normalized_x_a"], c["normalized_y_a"] = a_xy
    c["normalized_x_b"], c["normalized_y_b"] = b_xy
    return c


def _seam(c, color6=None, vig3=None):
    cams, models = F.tables(c)
    color6 = np.zeros((len(cams), 6)) if color6 is None else color6
    vig3 = np.zeros((len(models), 3)) if vig3 is None else vig3
    return host.color_balance_evaluate(c, cams, color6, models, vig3)


# ---- 1. the reference's unit tests -----------------------------------------------------------------------------------------
def test_match_cost_known_answers():
    """residuals 0 / 20 / 0 / -5 and the slope cases: inside Huber's quadratic zone (|r| <= 5) the gradient of camera a's
    L offset is -r and the cost r^2 / 2; at r = 20 the cost is 5 * 20 - 12.5 and the gradient -rho' r = -5"""
    e = _seam(_one((128, 128, 128), (128, 128, 128), r=(0.5, 0.5), th=(0.1, 0.1)))
    assert e["cost"] == 0.0 and not e["Jtr"].any()
    e = _seam(_one((150, 128, 128), (130, 128, 128)))
    assert e["cost"] == 5.0 * 20.0 - 12.5
    assert e["Jtr"][e["cam_col"][0]] == pytest.approx(-5.0, abs=1e-12) and e["Jtr"][e["cam_col"][1]] == pytest.approx(5.0, abs=1e-12)
    # offsets 15 and -5 correct the difference of 20
    e = _seam(_one((150, 128, 128), (130, 128, 128)), color6=[[15, 0, 0, 0, 0, 0], [-5, 0, 0, 0, 0, 0]])
    w2 = 0.01  # the priors' part: weight^2 = 0.01 at one appearance
    assert e["cost"] == pytest.approx(0.5 * w2 * (225 + 25), rel=1e-14)
    assert e["Jtr"][e["cam_col"][0]] == pytest.approx(w2 * 15, rel=1e-14)
    # slope 10 on both: 130 - 10 * 0.5 = 125 = 120 - 10 * (-0.5)
    e = _seam(_one((130, 128, 128), (120, 128, 128), a_xy=(0.5, 0), b_xy=(-0.5, 0)), color6=[[0, 0, 0, 0, 10, 0], [0, 0, 0, 0, 10, 0]])
    assert e["cost"] == pytest.approx(0.5 * w2 * 200, rel=1e-14)  # no match residual left
    assert e["Jtr"][e["cam_col"][0]] == pytest.approx(0.0, abs=1e-10)
    # slope 5 on both, nx 0.8 / -0.2: corr_a = 96, corr_b = 101, residual -5
    e = _seam(_one((100, 128, 128), (100, 128, 128), a_xy=(0.8, 0), b_xy=(-0.2, 0)), color6=[[0, 0, 0, 0, 5, 0], [0, 0, 0, 0, 5, 0]])
    assert -e["Jtr"][e["cam_col"][0]] == pytest.approx(-5.0, abs=1e-6)
    assert e["cost"] == pytest.approx(12.5 + 0.5 * w2 * 50, abs=1e-5)


def test_prior_known_answers():
    """ExposurePrior(0.5) on (10, -5, 3): residuals 5, -2.5, 1.5; VignettingPrior(0.1) on (1, 2, 3): 0.1, 0.2, 0.3 - read
    off the seam as gradient / weight, with the match residuals made zero"""
    # 25 correspondences: camera 1 appears 25 times, weight 0.1 * sqrt(25) = 0.5; lab_a - offset_a = lab_b
    c = _one((60, -5, 23), (50, 0, 20), models=(7, 8), n=25)
    e = _seam(c, color6=[[10, -5, 3, 0, 0, 0], [0, 0, 0, 0, 0, 0]])
    col = e["cam_col"][0]
    assert np.allclose(e["Jtr"][col:col + 3] / 0.5, [5.0, -2.5, 1.5], rtol=1e-15, atol=0)
    assert e["cost"] == pytest.approx(0.5 * (25 + 6.25 + 2.25), rel=1e-15)
    # one correspondence with two models: each model appears once, weight 0.1; radius 0: no vignetting in the residual
    c = _one((50, 0, 20), (50, 0, 20), models=(7, 8))
    e = _seam(c, vig3=[[1, 2, 3], [0, 0, 0]])
    col = e["model_col"][0]
    assert np.allclose(e["Jtr"][col:col + 3] / 0.1, [0.1, 0.2, 0.3], rtol=1e-15, atol=0)
    # a shared model appears twice per correspondence: weight 0.1 * sqrt(2)
    e = _seam(_one((50, 0, 20), (50, 0, 20)), vig3=[[1, 2, 3]])
    assert np.allclose(e["Jtr"][e["model_col"][0]:][:3], 0.02 * np.array([1.0, 2, 3]), rtol=1e-14, atol=0)


def test_solve_synthetic_exposure_difference():
    rng = np.random.default_rng(42)
    c = F.make_corr(200)
    true_l = 100.0 + np.arange(200) % 50
    c["lab_a"] = np.stack([true_l + 10, np.full(200, 128.0), np.full(200, 128.0)], 1)
    c["lab_b"] = np.stack([true_l - 5, np.full(200, 128.0), np.full(200, 128.0)], 1)
    c["camera_id_a"], c["camera_id_b"], c["model_id_a"], c["model_id_b"] = 100, 200, 1, 1
    c["normalized_radius_a"], c["normalized_radius_b"] = rng.uniform(0, 1, 200), rng.uniform(0, 1, 200)
    c["view_angle_a"] = c["view_angle_b"] = 0.1
    r = host.color_balance_solve(c)
    assert r["success"]
    assert r["per_image"][100]["lab_offset"][0] - r["per_image"][200]["lab_offset"][0] == pytest.approx(15.0, abs=1.0)


def test_solve_three_cameras():
    parts = []
    for (a, b), d in (((1, 2), 8.0), ((2, 3), 4.0)):
        c = F.make_corr(100)
        true_l = 80.0 + np.arange(100) % 40
        c["lab_a"] = np.stack([true_l + d, np.full(100, 128.0), np.full(100, 128.0)], 1)
        c["lab_b"] = np.stack([true_l, np.full(100, 128.0), np.full(100, 128.0)], 1)
        c["camera_id_a"], c["camera_id_b"], c["model_id_a"], c["model_id_b"] = a, b, 1, 1
        c["normalized_radius_a"] = c["normalized_radius_b"] = 0.3
        c["view_angle_a"] = c["view_angle_b"] = 0.05
        parts.append(c)
    r = host.color_balance_solve(np.concatenate(parts))
    assert r["success"]
    off = {k: v["lab_offset"][0] for k, v in r["per_image"].items()}
    assert off[1] - off[2] == pytest.approx(8.0, abs=1.5)
    assert off[2] - off[3] == pytest.approx(4.0, abs=1.5)


def test_solve_synthetic_directional_slope():
    rng = np.random.default_rng(123)
    n, slope_x = 400, 8.0
    c = F.make_corr(n)
    nx_a, ny_a, nx_b, ny_b = (rng.uniform(-0.9, 0.9, n).astype(np.float32) for _ in range(4))
    true_l = 100.0 + np.arange(n) % 30
    c["lab_a"] = np.stack([true_l + slope_x * nx_a, np.full(n, 128.0), np.full(n, 128.0)], 1)
    c["lab_b"] = np.stack([true_l, np.full(n, 128.0), np.full(n, 128.0)], 1)
    c["camera_id_a"], c["camera_id_b"], c["model_id_a"], c["model_id_b"] = 10, 20, 1, 1
    c["normalized_radius_a"] = c["normalized_radius_b"] = 0.3
    c["view_angle_a"] = c["view_angle_b"] = 0.05
    c["normalized_x_a"], c["normalized_y_a"], c["normalized_x_b"], c["normalized_y_b"] = nx_a, ny_a, nx_b, ny_b
    r = host.color_balance_solve(c)
    assert r["success"]
    a, b = r["per_image"][10]["slope"], r["per_image"][20]["slope"]
    assert a[0] - b[0] == pytest.approx(slope_x, abs=2.0)
    assert a[1] == pytest.approx(0.0, abs=2.0) and b[1] == pytest.approx(0.0, abs=2.0)


def test_solve_empty_and_edge_cases():
    r = host.color_balance_solve(F.make_corr(0))
    assert r["success"] is False and r["per_image"] == {} and r["per_model"] == {}
    # a non-finite observation: Ceres fails at iteration 0, the parameters stay 0, the gauge step still runs
    c = F.nonfinite_case()
    cams, _ = F.tables(c)
    r = host.color_balance_solve(c, positions={int(k): (float(i), float(i * i)) for i, k in enumerate(cams)})
    assert r["success"] is False and r["num_iterations"] == 0
    assert all(v["lab_offset"] == (0.0, 0.0, 0.0) and v["brdf"] == 0.0 and v["slope"] == (0.0, 0.0) for v in r["per_image"].values())
    # a correspondence of a camera with itself: a duplicate parameter block in Ceres; refused
    with pytest.raises(capi.OchipError, match="with itself"):
        host.color_balance_solve(_one((1, 2, 3), (1, 2, 3), cams=(5, 5)))
    # the result is ortho_blend's table
    r = host.color_balance_solve(F.scene(F.chain_pairs(3), 20, [0] * 3, 5))
    ids, six, mids, vig = host._color_tables(r)
    assert six.shape == (3, 6) and vig.shape == (1, 3) and list(mids) == [0]


# ---- 2. against the oracle's Ceres restatement ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("color_balance_oracle"))
    return F.build_driver(tmp), tmp


@pytest.mark.parametrize("name", sorted(F.solve_cases()))
def test_cpu_route_against_the_oracle(driver, name):
    exe, tmp = driver
    corr = F.solve_cases()[name]
    y = F.run_driver(exe, corr, tmp, name)
    assert y["success"]
    near = F.thresholds_clear(y)
    assert not near, f"fixture {name} is not usable: {near}"
    print(f"yardstick {name}: {y['num_iterations']} iterations, {y['message']!r}, last |dcost|/cost "
          f"{abs(y['iterations'][-1]['cost_change']) / y['iterations'][-2]['cost']:.3e}")
    got = host.color_balance_solve(corr)  # (no positions: before the gauge step, as the yardstick)
    F.compare_solution(got, y, f"cpu vs live yardstick, {name}")
    # the recorded results are this yardstick's
    rec = F.golden(name)
    assert rec["checksum"] == F.checksum(corr), "the fixture's correspondences changed: run scripts/make_color_balance_golden.py"
    F.compare_solution(got, rec, f"cpu vs recorded yardstick, {name}")
    assert rec["num_iterations"] == y["num_iterations"] and rec["message"] == y["message"]


def test_yardstick_does_not_depend_on_the_order(driver):
    """reordering the correspondences moves the yardstick's parameters by rounding only"""
    exe, tmp = driver
    corr = F.solve_cases()["chain40_seed1"]
    a = F.golden("chain40_seed1")
    b = F.run_driver(exe, corr[np.random.default_rng(3).permutation(len(corr))], tmp, "permuted")
    d = max(float(np.max(np.abs(np.array(a["per_image"][k]) - np.array(b["per_image"][k])))) for k in a["per_image"])
    print(f"yardstick, correspondences permuted: parameters move by {d:.3e}")
    assert d < 1e-9 and a["num_iterations"] == b["num_iterations"]


def test_grid_against_the_recorded_yardstick():
    corr = F.grid_case()
    rec = F.golden("grid20x20")
    assert rec["checksum"] == F.checksum(corr)
    assert not F.thresholds_clear(rec)
    F.compare_solution(host.color_balance_solve(corr), rec, "cpu vs recorded yardstick, grid20x20")


# ---- 3. gauge removal -------------------------------------------------------------------------------------------------------------
def _lstsq_detrend(xy, off):
    A = np.column_stack([xy, np.ones(len(xy))])
    sol, _, rank, sv = np.linalg.lstsq(A, off, rcond=None)  # rcond: epsilon * max(M, N), the library's threshold
    return off - A @ sol, rank, sv


@pytest.mark.parametrize("case", ["generic", "collinear", "collinear_axis", "coincident"])
def test_gauge_removal_against_lstsq(case):
    """Tolerance: both sides solve the same n x 3 least-squares problem backward-stably; the fitted VALUES A x differ by at
    most ~ n u cond(A) |b| when the rank decision is clear, where cond is taken over the singular values kept.  The
    positions below are O(100) around an O(1000) origin: cond(A) ~ 1e4 at full rank, and the bound used is
    64 n u cond |b|, about 1e-9 for |b| ~ 20."""
    rng = np.random.default_rng(7)
    n = 37
    t = rng.uniform(-100, 100, n)
    xy = dict(generic=np.column_stack([1000 + rng.uniform(-100, 100, n), 2000 + rng.uniform(-100, 100, n)]),
              collinear=np.column_stack([1000 + 3 * t, 2000 - 2 * t]),
              collinear_axis=np.column_stack([1000 + t, np.full(n, 2000.0)]),
              coincident=np.tile([[1000.0, 2000.0]], (n, 1)))[case]
    if case == "collinear":  # exactly collinear in fp64: integer parameters
        t = np.round(t)
        xy = np.column_stack([1000 + 3 * t, 2000 - 2 * t])
    off = rng.normal(0, 20, (n, 3))
    want, rank, sv = _lstsq_detrend(xy, off)
    got, my_rank = host.color_balance_remove_gauge(xy, off)
    assert my_rank == rank == dict(generic=3, collinear=2, collinear_axis=2, coincident=1)[case]
    cond = sv[0] / sv[rank - 1]
    tol = 64 * n * F.U * cond * np.abs(off).max()
    print(f"gauge {case}: rank {rank}, cond {cond:.3e}, worst difference {np.abs(got - want).max():.3e}, tolerance {tol:.3e}")
    assert np.abs(got - want).max() <= tol


def test_gauge_needs_three_positioned_cameras_and_skips_ids_without_a_position():
    corr = F.scene(F.chain_pairs(6), 60, [2] * 6, 8)
    cams, _ = F.tables(corr)
    raw = host.color_balance_solve(corr)
    pos = {int(k): (10.0 * i + (i % 2), 3.0 * i * i) for i, k in enumerate(cams)}
    # fewer than 3 positioned cameras: untouched; positions of ids the solve does not know are ignored
    two = host.color_balance_solve(corr, positions={**{k: pos[k] for k in list(pos)[:2]}, 1: (0, 0), 2: (5, 5)})
    assert two["per_image"] == raw["per_image"]
    # four of six positioned: those four lose their plane, the other two keep their offsets
    some = list(pos)[1:5]
    part = host.color_balance_solve(corr, positions=[(k, *pos[k]) for k in some])
    xy = np.array([pos[k] for k in some])
    off = np.array([raw["per_image"][k]["lab_offset"] for k in some])
    want, _, _ = _lstsq_detrend(xy, off)
    got = np.array([part["per_image"][k]["lab_offset"] for k in some])
    assert np.abs(got - want).max() <= 1e-9
    for k in set(pos) - set(some):
        assert part["per_image"][k] == raw["per_image"][k]
    for k in some:  # only the offsets move
        assert part["per_image"][k]["brdf"] == raw["per_image"][k]["brdf"] and part["per_image"][k]["slope"] == raw["per_image"][k]["slope"]
    assert part["per_model"] == raw["per_model"] and part["final_cost"] == raw["final_cost"]


def test_gauge_reads_the_graph_positions():
    from ortho_fixtures import make_graph, three_cameras

    pos, ori, model, _ = three_cameras()
    g = make_graph(pos, ori, model)
    ids = [int(i) for i in g.node_table()["id"]]
    corr = F.scene([(0, 1), (1, 2), (0, 2)], 80, [0] * 3, 9, ids=ids)
    raw = host.color_balance_solve(corr)
    got = host.color_balance_solve(corr, graph=g)
    xy = np.array(pos, np.float64)[:, :2]
    order = sorted(range(3), key=lambda i: ids[i])
    off = np.array([raw["per_image"][ids[i]]["lab_offset"] for i in order])
    want, _, _ = _lstsq_detrend(xy[order], off)
    assert np.abs(np.array([got["per_image"][ids[i]]["lab_offset"] for i in order]) - want).max() <= 1e-9
    g.close()


# ---- 4. the evaluation against long double -----------------------------------------------------------------------------------------
def test_cpu_evaluation_against_long_double():
    worst = dict(cost=0.0, JtJ=0.0, Jtr=0.0)
    for name, (corr, seed) in F.eval_cases().items():
        cams, models, c6, v3 = F.eval_state(corr, seed)
        ref = F.evaluate_longdouble(corr, cams, models, c6, v3)
        got = F.canonical(host.color_balance_evaluate(corr, cams, c6, models, v3), len(cams), len(models))
        r = F.eval_ratios(got, ref)
        print(f"COLOR_BALANCE_EVAL_RATIOS cpu {name} (c = 1): {json.dumps(r)}")
        for k in worst:
            worst[k] = max(worst[k], r[k])
    print(f"COLOR_BALANCE_EVAL_RATIOS cpu worst (c = 1): {json.dumps(worst)}; C_BOUND = {F.C_BOUND}")
    # C_BOUND derives from the ratio recorded in the fixtures file (next power of two at or above 8 x it); a run on another
    # toolchain may measure a somewhat different ratio and must still leave the device its margin of 8
    assert F.C_BOUND == 2.0 ** int(np.ceil(np.log2(8 * max(F.MEASURED_RATIO_C1.values()))))
    assert max(worst.values()) <= F.C_BOUND / 8


def test_cost_only_evaluation_equals_the_full_one():
    corr, seed = F.eval_cases()["mixed_models"]
    cams, models, c6, v3 = F.eval_state(corr, seed)
    assert host.color_balance_evaluate(corr, cams, c6, models, v3, jacobian=False)["cost"] == \
        host.color_balance_evaluate(corr, cams, c6, models, v3)["cost"]


def test_device_plan_run_on_the_host_against_long_double():
    """The device's evaluation - its plan (chunks of 64, reverse Cuthill-McKee and dissected camera order, owners' record
    lists) and its kernels' arithmetic in their order, csrc/color_balance_plan.hpp - run on the host: within the same
    bounds of the long-double restatement, on the evaluation scenes and on the 20 x 20 grid, whose plan has regions and
    separator cameras.  tests/test_gpu_color_balance.py holds the device to this run bit for bit."""
    for name, (corr, seed) in [*F.eval_cases().items(), ("grid20x20", (F.grid_case(), 5))]:
        cams, models, c6, v3 = F.eval_state(corr, seed)
        ref = F.evaluate_longdouble(corr, cams, models, c6, v3)
        ev = host.color_balance_evaluate(corr, cams, c6, models, v3, plan=True)
        r = F.eval_ratios(F.canonical(ev, len(cams), len(models)), ref)
        print(f"COLOR_BALANCE_EVAL_RATIOS device plan on the host, {name} (c = 1): {json.dumps(r)}; layout {ev['layout']}")
        assert max(r.values()) <= F.C_BOUND, (name, r)
        assert host.color_balance_evaluate(corr, cams, c6, models, v3, plan=True, jacobian=False)["cost"] == ev["cost"]
        # every unknown has its own column
        cols = np.concatenate([(ev["cam_col"][:, None] + np.arange(6)).ravel(), (ev["model_col"][:, None] + np.arange(3)).ravel()])
        assert sorted(cols) == list(range(6 * len(cams) + 3 * len(models)))
        if name == "grid20x20":
            assert ev["layout"]["regions"] > 1 and ev["layout"]["separators"] > 0 and ev["layout"]["tail_begin"] % 64 != 0
        if name == "multi_block_tail_and_band":
            assert ev["layout"]["tail_begin"] >= 128 and 6 * len(cams) + 3 * len(models) - ev["layout"]["tail_begin"] >= 64


def test_ortho_mosaic_solve_on_the_cpu_route():
    """ortho_mosaic(color_balance="solve") = layers pass for the correspondences, color_balance_solve, then the usual pass
    with the tables; None and a dict behave as before"""
    from layers_fixtures import four_camera_scene

    g, s, _ = four_camera_scene(seed=4)
    imgs = F.smooth_images(4, 120, 160)
    plan, cfg = F.MOSAIC_PLAN, F.MOSAIC_CONFIG
    lcfg = {k: v for k, v in cfg.items() if k in host.LAYERS_CONFIG}
    solved = host.ortho_mosaic(plan, g, [s], imgs, config=cfg, color_balance="solve", tile_rows=2)
    corr = []
    for row0 in range(0, plan["height"], 64):
        dsm = host.dsm_render(plan, [s], row0=row0, rows=min(64, plan["height"] - row0))
        corr.append(host.ortho_layers(plan, g, [s], imgs, row0=row0, tile_rows=2, config=lcfg, dsm=dsm)["correspondences"])
    corr = np.concatenate(corr)
    assert len(corr) > 200
    tables = host.color_balance_solve(corr, graph=g)
    assert tables["success"]
    assert np.array_equal(solved, host.ortho_mosaic(plan, g, [s], imgs, config=cfg, color_balance=tables, tile_rows=2))
    plain = host.ortho_mosaic(plan, g, [s], imgs, config=cfg, tile_rows=2)
    assert np.array_equal(plain, host.ortho_mosaic(plan, g, [s], imgs, config=cfg, color_balance=None, tile_rows=2))
    assert not np.array_equal(plain, solved)
    # the two brighter images (nodes 1 and 2, on one diagonal) come out with the larger L offsets
    ids = [int(i) for i in g.node_table()["id"]]
    off = [tables["per_image"][i]["lab_offset"][0] for i in ids]
    print("mosaic, cpu route: L offsets", off, "correspondences", len(corr), "iterations", tables["num_iterations"])
    assert min(off[1], off[2]) > max(off[0], off[3])
    with pytest.raises(ValueError):
        host.ortho_mosaic(plan, g, [s], imgs, config=cfg, color_balance="balance")
    g.close()

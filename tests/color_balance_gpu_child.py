"""The scenarios of test_gpu_color_balance.py, run in a child process (as blend_gpu_child.py, torch first): the device
engine of the colour-balance solve (csrc/color_balance.hip) against the long-double evaluation, the CPU route run live
and the recorded yardstick results.  `python color_balance_gpu_child.py <tests dir> <repo dir>` runs every scenario and
prints one JSON line {scenario: "ok" or the failure's traceback}; the figures it measures go to stderr."""
import json
import sys
import time
import traceback

import numpy as np
import torch

torch.cuda.init()
if __name__ == "__main__":
    sys.path[:0] = sys.argv[1:3]

import color_balance_fixtures as F  # noqa: E402
from layers_fixtures import four_camera_scene  # noqa: E402
from opencalibration_amd import capi, host  # noqa: E402


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def scenario_evaluation(ctx, name):
    corr, seed = F.eval_cases()[name] if name != "grid20x20" else (F.grid_case(), 5)
    cams, models, c6, v3 = F.eval_state(corr, seed)
    ref = F.evaluate_longdouble(corr, cams, models, c6, v3)
    ev = host.color_balance_evaluate(corr, cams, c6, models, v3, ctx=ctx)
    assert not ev["failed"]
    r = F.eval_ratios(F.canonical(ev, len(cams), len(models)), ref)
    log(f"COLOR_BALANCE_EVAL_RATIOS device {name} (c = 1): {json.dumps(r)}; C_BOUND = {F.C_BOUND}")
    assert max(r.values()) <= F.C_BOUND, r
    # the plan's evaluation run on the host (color_balance_plan.hpp) defines what the device computes: bit for bit
    hostrun = host.color_balance_evaluate(corr, cams, c6, models, v3, plan=True)
    log(f"device layout {name}: {hostrun['layout']}")
    assert np.array_equal(hostrun["cam_col"], ev["cam_col"]) and np.array_equal(hostrun["model_col"], ev["model_col"])
    assert hostrun["cost"] == ev["cost"], (hostrun["cost"], ev["cost"])
    assert np.array_equal(hostrun["JtJ"], ev["JtJ"]) and np.array_equal(hostrun["Jtr"], ev["Jtr"])
    # the cost-only kernel sums the same terms in the same order
    assert host.color_balance_evaluate(corr, cams, c6, models, v3, ctx=ctx, jacobian=False)["cost"] == ev["cost"]
    again = host.color_balance_evaluate(corr, cams, c6, models, v3, ctx=ctx)
    assert again["cost"] == ev["cost"] and np.array_equal(again["JtJ"], ev["JtJ"]) and np.array_equal(again["Jtr"], ev["Jtr"])


def solve_and_compare(ctx, corr, name, rec):
    t0 = time.perf_counter()
    dev = host.color_balance_solve(corr, ctx=ctx)
    t1 = time.perf_counter()
    cpu = host.color_balance_solve(corr)
    t2 = time.perf_counter()
    log(f"{name}: device {t1 - t0:.3f} s, cpu route {t2 - t1:.3f} s")
    F.compare_solution(dev, F.as_yardstick(cpu), f"device vs cpu route, {name}")
    assert rec["checksum"] == F.checksum(corr)
    assert not F.thresholds_clear(rec)
    F.compare_solution(dev, rec, f"device vs recorded yardstick, {name}")
    again = host.color_balance_solve(corr, ctx=ctx)
    assert again == dev, "two device solves of one input differ"


def scenario_solve(ctx, name):
    solve_and_compare(ctx, F.solve_cases()[name], name, F.golden(name))


def scenario_grid(ctx):
    solve_and_compare(ctx, F.grid_case(), "grid20x20", F.golden("grid20x20"))


def scenario_status_only(ctx):
    r = host.color_balance_solve(F.make_corr(0), ctx=ctx)
    assert r["success"] is False and r["per_image"] == {} and r["per_model"] == {}
    c = F.nonfinite_case()
    cams, _ = F.tables(c)
    r = host.color_balance_solve(c, ctx=ctx, positions={int(k): (float(i), float(i * i)) for i, k in enumerate(cams)})
    assert r["success"] is False and r["num_iterations"] == 0
    assert all(v["lab_offset"] == (0.0, 0.0, 0.0) and v["brdf"] == 0.0 for v in r["per_image"].values())
    assert r == host.color_balance_solve(c, positions={int(k): (float(i), float(i * i)) for i, k in enumerate(cams)})
    bad = F.make_corr(1)
    bad["camera_id_a"] = bad["camera_id_b"] = 5
    try:
        host.color_balance_solve(bad, ctx=ctx)
    except capi.OchipError as e:
        assert "with itself" in str(e)
    else:
        raise AssertionError("a correspondence of a camera with itself was accepted")
    # the context still solves afterwards
    scenario_solve(ctx, "ids_near_2_63")


def scenario_mosaic_solve(ctx):
    g, s, _ = four_camera_scene(seed=4)
    imgs = F.smooth_images(4, 120, 160)
    plan, cfg = F.MOSAIC_PLAN, F.MOSAIC_CONFIG
    dimg = [torch.from_numpy(im).to("cuda:0") for im in imgs]
    lcfg = {k: v for k, v in cfg.items() if k in host.LAYERS_CONFIG}
    with host.OrthoMesh(ctx, [s]) as mesh:
        solved = host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, color_balance="solve", tile_rows=2).cpu().numpy()
        corr = np.concatenate([b["correspondences"] for b in host.ortho_layers_bands(plan, g, [s], dimg, mesh=mesh, tile_rows=2,
                                                                                    config=lcfg)])
        assert len(corr) > 200, len(corr)
        tables = host.color_balance_solve(corr, graph=g, ctx=ctx)
        assert tables["success"]
        given = host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, color_balance=tables, tile_rows=2).cpu().numpy()
        assert np.array_equal(solved, given)
        plain = host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, color_balance=None, tile_rows=2).cpu().numpy()
        today = host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, tile_rows=2).cpu().numpy()
        assert np.array_equal(plain, today)
        assert not np.array_equal(plain, solved), "the solved tables change nothing"
    cpu = host.color_balance_solve(corr, graph=g)
    F.compare_solution(tables, F.as_yardstick(cpu), "mosaic tables, device vs cpu route")
    # the brighter images get the larger L offsets
    ids = [int(i) for i in g.node_table()["id"]]
    off = [tables["per_image"][i]["lab_offset"][0] for i in ids if i in tables["per_image"]]
    log("mosaic: L offsets", off, "correspondences", len(corr), "iterations", tables["num_iterations"])
    g.close()


SCENARIOS = {
    **{f"evaluation_{k}": (lambda ctx, k=k: scenario_evaluation(ctx, k)) for k in [*F.eval_cases(), "grid20x20"]},
    **{f"solve_{k}": (lambda ctx, k=k: scenario_solve(ctx, k)) for k in F.solve_cases()},
    "solve_grid20x20": scenario_grid,
    "status_only_cases": scenario_status_only,
    "mosaic_solve": scenario_mosaic_solve,
}

if __name__ == "__main__":
    ctx = capi.Context(0)
    res = {}
    stopped = None
    for name, fn in SCENARIOS.items():
        if stopped:
            res[name] = f"not run: the device reported an error in {stopped}"
            continue
        t0 = time.perf_counter()
        try:
            fn(ctx)
            res[name] = "ok"
        except capi.OchipError:  # a HIP or library error: nothing more is started on this device
            res[name] = traceback.format_exc()
            stopped = name
        except Exception:  # a comparison failed: the device is fine
            res[name] = traceback.format_exc()
        log(f"scenario {name}: {time.perf_counter() - t0:.2f} s")
    ctx.close()
    print(json.dumps(res))

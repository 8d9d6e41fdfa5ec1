"""The colour-balance solve on C3 geometry (the scene of probe_ortho_blend.py: the cameras of synth.make_grid(40, 25),
the rebuilt and perturbed mesh, the 1 000 views rendered into HBM, 2 layers): one pass of the layered render over the
raster collects the correspondences, then color_balance_solve runs on the device.  Prints one JSON line: the
correspondence count, unknowns and iterations, the solve's wall time (best of 3), the CPU route on the largest prefix
of the cameras it holds (4 096 unknowns) against the device on the same input, and the yardstick's time on that input
when --yardstick (the oracle's driver, built with g++) is given.  --quick: one device solve (the kernel-trace run).
Needs the GPU."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opencalibration_amd import capi, host, pipeline, synth  # noqa: E402


def main():
    import torch

    torch.cuda.init()  # torch's HIP runtime comes up before libochip.so is loaded (as in bench.py)
    quick = "--quick" in sys.argv
    grid = synth.make_grid(40, 25, feats=16)
    pos = np.ascontiguousarray(grid.position, np.float64)
    rng = np.random.default_rng(0)
    surface = host.rebuild_mesh(pos)
    v = surface.arrays()["vertices"]
    surface.set_heights(v[:, 2] - grid.meta.get("height", 100.0) + rng.uniform(-2, 2, len(v)))
    g = host.Graph()
    m = g.add_model(np.asarray(grid.model, np.float64))
    for p in pos:
        g.add_image(np.zeros((0, 2)), np.zeros(0, np.float32), np.zeros((0, 8), np.uint64), 0, m, p)
    g.set_orientations(np.ascontiguousarray(grid.orientation, np.float64))
    ctx = capi.Context(0)
    W_img, H_img = int(grid.model[8]), int(grid.model[9])
    views, _ = pipeline.synthetic_views(ctx, grid)
    ptrs = [int(views) + i * W_img * H_img * 3 for i in range(len(pos))]
    plan = host.dsm_plan(g, [surface])
    mesh = host.OrthoMesh(ctx, [surface])
    t0 = time.perf_counter()
    corr = np.concatenate([b["correspondences"] for b in host.ortho_layers_bands(plan, g, [surface], ptrs, mesh=mesh)])
    layers_s = time.perf_counter() - t0
    n_cams = len(np.unique(np.concatenate([corr["camera_id_a"], corr["camera_id_b"]])))
    n_models = len(np.unique(np.concatenate([corr["model_id_a"], corr["model_id_b"]])))
    out = dict(images=len(pos), device=ctx.device_info()["name"], width=plan["width"], height=plan["height"],
               correspondences=int(len(corr)), cameras=n_cams, models=n_models, unknowns=6 * n_cams + 3 * n_models,
               layers_pass_s=layers_s)

    def solve(c, on_device=True):
        t0 = time.perf_counter()
        r = host.color_balance_solve(c, graph=g, ctx=ctx if on_device else None)
        return time.perf_counter() - t0, r

    times = [solve(corr) for _ in range(1 if quick else 3)]
    r = times[0][1]
    out.update(solve_s=min(t for t, _ in times), solve_s_all=[t for t, _ in times], iterations=r["num_iterations"],
               success=r["success"], final_cost=r["final_cost"], termination=r["termination"],
               reruns_equal=all(x == r for _, x in times))
    if not quick:
        # the CPU route's largest input: the correspondences among the first cameras that fit 4 096 unknowns
        ids = np.unique(np.concatenate([corr["camera_id_a"], corr["camera_id_b"]]))[:(4096 - 3 * n_models) // 6]
        sub = corr[np.isin(corr["camera_id_a"], ids) & np.isin(corr["camera_id_b"], ids)]
        cpu_s, cpu = solve(sub, on_device=False)
        dev_s, dev = solve(sub)
        worst = max(float(np.max(np.abs(np.array([*cpu["per_image"][k]["lab_offset"], cpu["per_image"][k]["brdf"], *cpu["per_image"][k]["slope"]]) -
                                        np.array([*dev["per_image"][k]["lab_offset"], dev["per_image"][k]["brdf"], *dev["per_image"][k]["slope"]]))))
                    for k in cpu["per_image"])
        out.update(cpu_cameras=len(cpu["per_image"]), cpu_correspondences=int(len(sub)), cpu_route_s=cpu_s, device_same_input_s=dev_s,
                   cpu_iterations=cpu["num_iterations"], device_same_input_iterations=dev["num_iterations"],
                   cpu_device_worst_parameter_difference=worst)
        if "--yardstick" in sys.argv:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import color_balance_fixtures as F

            with tempfile.TemporaryDirectory() as tmp:
                exe = F.build_driver(tmp)
                F.write_problem(os.path.join(tmp, "p.txt"), sub)
                t0 = time.perf_counter()
                y = F.run_driver(exe, sub, tmp, "p")
                out.update(yardstick_s=time.perf_counter() - t0, yardstick_iterations=y["num_iterations"])
    mesh.close()
    ctx.synth_views_free(views)
    g.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

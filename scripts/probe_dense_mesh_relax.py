"""DENSE_MESH_RELAX at the size of the bench's C3 survey: the points-per-triangle count and the
whole state by the device route and by the host route (och_count_points_per_triangle: locate under OpenMP, sums on one
thread), alternating in one process, best of three with all runs listed.

The cloud is not the one Graph.densify_mesh leaves - getting there runs the whole pipeline - but 650 000 points sampled over
rolling ground with noise, under a grid of 8 x 8 cameras 50 m up; the state refines the minimal mesh to about 10^4
triangles.  Usage: probe_dense_mesh_relax.py [--points N] [--out FILE] [--state-only]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from opencalibration_amd import capi, host

MODEL_600 = np.array([600.0, 400, 300, 0, 0, 0, 0, 0, 800, 600])
DOWN = np.array([1.0, 0.0, 0.0, 0.0]) * np.sin(np.pi / 2) + np.array([0, 0, 0, np.cos(np.pi / 2)])


def scene(n_points, seed=1):
    rng = np.random.default_rng(seed)
    rows = cols = 8
    spacing, height = 25.0, 50.0
    pos = np.array([[c * spacing, r * spacing, height] for r in range(rows) for c in range(cols)])
    ground = lambda x, y: 3.0 * np.sin(x / 15.0) * np.cos(y / 18.0)
    xy = rng.uniform(-0.5 * spacing, (cols - 0.5) * spacing, (n_points, 2))
    cloud = np.concatenate([xy, (ground(xy[:, 0], xy[:, 1]) + rng.normal(0, 0.25, n_points))[:, None]], axis=1)
    g = host.Graph()
    m = g.add_model(MODEL_600)
    for p in pos:
        g.add_image(np.zeros((0, 2)), np.zeros(0, np.float32), np.zeros((0, 8), np.uint64), 0, m, p)
    g.set_orientations(np.array([DOWN for _ in pos]))
    return g, pos, cloud


def start_surface(pos, cloud):
    s = host.rebuild_mesh(pos, minimal=True)
    s.set_clouds([cloud])
    return s


def timed(f):
    t = time.perf_counter()
    r = f()
    return time.perf_counter() - t, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=650000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--state-only", action="store_true", help="one state on the device and nothing else (for a kernel trace)")
    a = ap.parse_args()
    ctx = capi.Context(0)
    g, pos, cloud = scene(a.points)
    if a.state_only:
        s, log = g.dense_mesh_relax(start_surface(pos, cloud), ctx=ctx)
        print("state: %d runs, %d vertices" % (len(log), log[-1]["vertices"]))
        return
    out = {"points": a.points, "device": ctx.device_info()["name"], "omp_threads": os.environ.get("OMP_NUM_THREADS"), "runs": {}}
    # the final mesh, by the host route
    final = start_surface(pos, cloud)
    _, log = g.dense_mesh_relax(final)
    first = start_surface(pos, cloud)
    out["state_runs"] = len(log)
    out["final_mesh"] = {"vertices": len(final.arrays()["vertices"]), "located_triangles": len(final.locate_table()["vertex_xy"])}
    out["first_mesh"] = {"vertices": len(first.arrays()["vertices"]), "located_triangles": len(first.locate_table()["vertex_xy"])}
    t_up, kept = timed(lambda: host.PointCounter(cloud, ctx=ctx))
    out["runs"]["upload_s"] = [t_up]
    cpu_flat = host.PointCounter(cloud)
    kept.count(first)                                   # (first use: module load, pool blocks)
    for name, surface in (("first", first), ("final", final)):
        dev, hst, flat = [], [], []
        for rep in range(3):
            td, rd = timed(lambda: kept.count(surface))
            th, rh = timed(lambda: surface.count_points_per_triangle())
            tf, rf = timed(lambda: cpu_flat.count(surface))
            assert all(np.array_equal(x, y) for x, y in zip(rd, rh)) and all(np.array_equal(x, y) for x, y in zip(rf, rh))
            dev.append(td), hst.append(th), flat.append(tf)
        out["runs"]["count_%s_mesh" % name] = {"device_s": dev, "host_s": hst, "flat_cpu_s": flat, "rows": len(rd[0])}
    dev, hst = [], []
    for rep in range(3):
        td, (sd, logd) = timed(lambda: g.dense_mesh_relax(start_surface(pos, cloud), ctx=ctx))
        th, (sh, logh) = timed(lambda: g.dense_mesh_relax(start_surface(pos, cloud)))
        assert logd == logh and np.array_equal(sd.arrays()["edges"], sh.arrays()["edges"])
        dev.append(td), hst.append(th)
    t_setup, _ = timed(lambda: start_surface(pos, cloud))
    out["runs"]["state"] = {"device_s": dev, "host_s": hst, "surface_setup_s_included": t_setup,
                            "log": [[int(r["above_threshold"]), int(r["created"]), int(r["vertices"])] for r in logd]}
    # smaller clouds: where the device stops winning
    sizes = {}
    for n in (1000, 10000, 100000):
        sub = cloud[:n]
        k = host.PointCounter(sub, ctx=ctx)
        final.set_clouds([sub])
        k.count(final)
        d = min(timed(lambda: k.count(final))[0] for _ in range(3))
        h = min(timed(lambda: final.count_points_per_triangle())[0] for _ in range(3))
        sizes[str(n)] = {"device_s": d, "host_s": h}
        k.close()
    out["runs"]["count_final_mesh_by_points"] = sizes
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    kept.close()
    ctx.close()


if __name__ == "__main__":
    main()

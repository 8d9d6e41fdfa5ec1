"""The per-tile progress thumbnails on C3 geometry: the scene of probe_ortho_blend.py - the cameras of
synth.make_grid(40, 25), the rebuilt and perturbed mesh, the 1 000 views rendered into HBM, 2 layers, tiles of 1 024, bands
of one tile row.  Writes profiles/tile_progress_probe.json:

  unchanged path   ortho_mosaic with progress=None in this tree against the same call in a build of the parent commit
                   (--old DIR: a checkout of it with its libraries built, e.g. `git archive <parent> | tar -x -C _ab_old`
                   and `python -m opencalibration_amd.build` there).  The two builds alternate, a process each, three runs
                   each; the verdict is whether the difference of the two medians lies inside the two builds' own spreads.
  progress on      ortho_mosaic with a callback that keeps every update, three runs, in one process with three more runs
                   without it.
  today            what a caller without this has to do for the same updates: per band download the layers, their weights
                   and the blended rows and run the CPU route; timed per band without the render, summed.  Its updates must
                   equal the callback's, bit for bit.

Every run is a process of its own that ends before the next starts; after one that fails nothing more is started.
--child MODE --tree DIR is such a process (MODE plain, progress, today, quick: one mosaic with progress, for the kernel
trace).  Needs the GPU."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scene(tree):
    sys.path.insert(0, tree)
    import numpy as np
    import torch

    torch.cuda.init()  # torch's HIP runtime comes up before libochip.so is loaded (as in bench.py)
    from opencalibration_amd import capi, host, pipeline, synth

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
    w_img, h_img = int(grid.model[8]), int(grid.model[9])
    views, _ = pipeline.synthetic_views(ctx, grid)
    ptrs = [int(views) + i * w_img * h_img * 3 for i in range(len(pos))]
    plan = host.dsm_plan(g, [surface])
    node_ids = host.ortho_layers_cameras(g, [surface])["node_ids"]
    crng = np.random.default_rng(1)
    cb = dict(per_image={int(n): dict(lab_offset=crng.normal(0, 2, 3), brdf=0.5, slope=crng.normal(0, 1, 2))
                         for n in node_ids[::2]}, per_model={0: (3.0, -1.0, 0.5)})
    mesh = host.OrthoMesh(ctx, [surface])
    mosaic = torch.empty((plan["height"], plan["width"], 4), dtype=torch.uint8, device="cuda:0")
    return dict(np=np, torch=torch, host=host, ctx=ctx, g=g, surface=surface, ptrs=ptrs, plan=plan, cb=cb, mesh=mesh, mosaic=mosaic,
                views=views)


def child(mode, tree):
    s = scene(tree)
    np, torch, host, plan = s["np"], s["torch"], s["host"], s["plan"]
    t = host.BLEND_CONFIG["tile_size"]
    out = dict(mode=mode, tree=os.path.basename(os.path.abspath(tree)), width=plan["width"], height=plan["height"], tile_size=t,
               device=s["ctx"].device_info()["name"])

    def mosaic(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host.ortho_mosaic(plan, s["g"], [s["surface"]], s["ptrs"], mesh=s["mesh"], color_balance=s["cb"], out=s["mosaic"], **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    if mode == "plain":
        mosaic()  # warms the pools and the allocator
        out["mosaic_s"] = mosaic()
    elif mode == "quick":
        got = []
        out["mosaic_progress_s"] = mosaic(progress=got.append)
        out["updates"] = len(got)
    elif mode == "progress":
        got = []
        mosaic(progress=got.append)
        plain, on = [], []
        for _ in range(3):
            plain.append(mosaic())
            got.clear()
            on.append(mosaic(progress=got.append))
        tiles = -(-plan["width"] // t) * -(-plan["height"] // t)
        out.update(mosaic_s_all=plain, mosaic_progress_s_all=on, updates=len(got), tiles=tiles,
                   thumbnail_bytes=int(sum(u["thumbnail"].nbytes for u in got)),
                   scales=sorted({u["scale"] for u in got}))
    elif mode == "today":
        got = []
        mosaic(progress=got.append)
        by_key = {(u["pass"], u["tile_index"]): u for u in got}
        dev, nl, w = "cuda:0", host.LAYERS_CONFIG["num_layers"], plan["width"]
        spent, equal, moved = 0.0, True, 0
        for row0 in range(0, plan["height"], t):
            rows = min(t, plan["height"] - row0)
            lay = dict(bgra=torch.empty((nl, rows, w, 4), dtype=torch.uint8, device=dev),
                       camera_id=torch.empty((nl, rows, w), dtype=torch.int64, device=dev),
                       weight=torch.empty((nl, rows, w), dtype=torch.float32, device=dev))
            host.ortho_layers(plan, s["g"], [s["surface"]], s["ptrs"], mesh=s["mesh"], row0=row0, tile_rows=1, out=lay)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bgra, weight, rgba = lay["bgra"].cpu().numpy(), lay["weight"].cpu().numpy(), s["mosaic"][row0:row0 + rows].cpu().numpy()
            ups = host.ortho_tile_updates(plan, bgra, 1, row0=row0, weight=weight) + host.ortho_tile_updates(plan, rgba, 2, row0=row0)
            spent += time.perf_counter() - t0
            moved += bgra.nbytes + weight.nbytes + rgba.nbytes
            for u in ups:
                d = by_key[(u["pass"], u["tile_index"])]
                equal = equal and np.array_equal(u["thumbnail"], d["thumbnail"]) and \
                    all(u[k] == d[k] for k in u if k != "thumbnail")
        out.update(today_s=spent, today_downloaded_bytes=moved, today_equals_callback=bool(equal), updates=len(got),
                   cpu_threads=os.environ.get("OMP_NUM_THREADS"))
    else:
        raise SystemExit(f"unknown mode {mode}")
    s["mesh"].close()
    s["ctx"].synth_views_free(s["views"])
    s["g"].close()
    s["ctx"].close()
    print(json.dumps(out), flush=True)


def run_child(mode, tree, limit=240):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--tree", tree], capture_output=True, text=True,
                       timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"{mode} in {tree} ended with {r.returncode}: nothing more is started\n{r.stdout[-1000:]}\n{r.stderr[-3000:]}")
    print(f"{mode} in {os.path.basename(os.path.abspath(tree))}: {r.stdout.strip().splitlines()[-1][:300]}", file=sys.stderr, flush=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    old = sys.argv[sys.argv.index("--old") + 1] if "--old" in sys.argv else None
    out = {}
    if old is not None:
        new_s, old_s = [], []
        for _ in range(3):
            new_s.append(run_child("plain", ROOT)["mosaic_s"])
            old_s.append(run_child("plain", old)["mosaic_s"])
        diff = statistics.median(new_s) - statistics.median(old_s)
        spread = max(max(new_s) - min(new_s), max(old_s) - min(old_s))
        out.update(unchanged_new_s_all=new_s, unchanged_parent_s_all=old_s, unchanged_difference_s=diff,
                   unchanged_spread_s=spread, unchanged_inside_spread=bool(abs(diff) <= spread))
    else:
        out["unchanged"] = "not measured: no build of the parent commit given (--old DIR)"
    p = run_child("progress", ROOT, limit=420)
    out.update({k: p[k] for k in ("device", "width", "height", "tile_size", "tiles", "updates", "thumbnail_bytes", "scales",
                                  "mosaic_s_all", "mosaic_progress_s_all")})
    out.update(mosaic_s=min(p["mosaic_s_all"]), mosaic_progress_s=min(p["mosaic_progress_s_all"]),
               progress_excess=min(p["mosaic_progress_s_all"]) / min(p["mosaic_s_all"]) - 1.0,
               plain_spread=(max(p["mosaic_s_all"]) - min(p["mosaic_s_all"])) / min(p["mosaic_s_all"]))
    t = run_child("today", ROOT, limit=900)
    out.update({k: t[k] for k in ("today_s", "today_downloaded_bytes", "today_equals_callback", "cpu_threads")})
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "tile_progress_probe.json"), "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(sys.argv[sys.argv.index("--child") + 1], sys.argv[sys.argv.index("--tree") + 1])
    else:
        main()

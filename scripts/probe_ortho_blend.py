"""The blended full-resolution orthomosaic on C3 geometry (the scene of probe_ortho_layers.py: the cameras of
synth.make_grid(40, 25), the rebuilt and perturbed mesh, the 1 000 views rendered into HBM), 2 layers, bands of one
1 024-row tile row.  Prints one JSON line: the blend's device time alone (the layers and DSM of each band rendered first,
outside the clock; best of 3 of the summed band calls), ortho_mosaic end to end into one device tensor (DSM -> layers ->
blend per band; best of 3), and the CPU route on one band of 64 rows at tile_size 64 against the device for the same call,
with their exact agreement.  --quick: one ortho_mosaic pass (the kernel-trace run).  Needs the GPU."""
import json
import os
import sys
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
    W, H = plan["width"], plan["height"]
    T, L = host.BLEND_CONFIG["tile_size"], host.LAYERS_CONFIG["num_layers"]
    node_ids = host.ortho_layers_cameras(g, [surface])["node_ids"]
    # a colour table: every other image offset and sloped, model 0 vignetted
    crng = np.random.default_rng(1)
    cb = dict(per_image={int(n): dict(lab_offset=crng.normal(0, 2, 3), brdf=0.5, slope=crng.normal(0, 1, 2))
                         for n in node_ids[::2]}, per_model={0: (3.0, -1.0, 0.5)})
    out = dict(images=len(pos), image_size=[W_img, H_img], device=ctx.device_info()["name"], width=W, height=H, layers=L,
               tile_size=T, bands=-(-H // T), gsd=plan["gsd"], color_entries=len(cb["per_image"]))
    mesh = host.OrthoMesh(ctx, [surface])
    dev = "cuda:0"
    mosaic = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)

    def blend_alone():
        total = 0.0
        for row0 in range(0, H, T):
            rows = min(T, H - row0)
            dsm = torch.empty((rows, W), dtype=torch.float32, device=dev)
            host.dsm_render(plan, [surface], mesh=mesh, row0=row0, rows=rows, out=dsm)
            lay = dict(bgra=torch.empty((L, rows, W, 4), dtype=torch.uint8, device=dev),
                       camera_id=torch.empty((L, rows, W), dtype=torch.int64, device=dev))
            r = host.ortho_layers(plan, g, [surface], ptrs, mesh=mesh, row0=row0, tile_rows=1, out=lay)
            lay["row0"] = r["row0"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host.ortho_blend(plan, g, [surface], lay, dsm, cb, ctx=ctx, out=mosaic[row0:row0 + rows])
            torch.cuda.synchronize()
            total += time.perf_counter() - t0
        return total

    def end_to_end():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host.ortho_mosaic(plan, g, [surface], ptrs, mesh=mesh, color_balance=cb, out=mosaic)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    if quick:
        out.update(mosaic_s=end_to_end())
    else:
        blend = [blend_alone() for _ in range(3)]
        e2e = [end_to_end() for _ in range(3)]
        a = mosaic[..., 3]
        out.update(blend_s=min(blend), blend_s_all=blend, mosaic_s=min(e2e), mosaic_s_all=e2e, gpx=W * H / 1e9,
                   blend_gpx_per_s=W * H / min(blend) / 1e9, opaque_fraction=float((a == 255).float().mean().item()))
        # one band of 64 rows at tile_size 64 by both routes, from the same device-rendered layers and heights
        small = dict(tile_size=64)
        r0 = (H // 2) // 64 * 64
        lay = host.ortho_layers(plan, g, [surface], ptrs, mesh=mesh, row0=r0, tile_rows=1, config=small)
        dsm = host.dsm_render(plan, [surface], mesh=mesh, row0=r0, rows=lay["rows"])
        t0 = time.perf_counter()
        d_rgba = host.ortho_blend(plan, g, [surface], lay, dsm, cb, ctx=ctx, config=small)
        dev_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        c_rgba = host.ortho_blend(plan, g, [surface], lay, dsm, cb, config=small)
        cpu_s = time.perf_counter() - t0
        out.update(cpu_band_rows=lay["rows"], cpu_band_px=lay["rows"] * W, cpu_band_s=cpu_s, device_band_s=dev_s,
                   cpu_threads=os.environ.get("OMP_NUM_THREADS"), band_rgba_equal=bool(np.array_equal(d_rgba, c_rgba)))
    mesh.close()
    ctx.synth_views_free(views)
    g.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

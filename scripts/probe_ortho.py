"""The orthomosaic preview and the full-resolution DSM on C3 geometry: the cameras of synth.make_grid(40, 25), the mesh
rebuilt under them (rebuildMesh) with perturbed heights, thumbnails of noise at 1/8 of the image size.  Prints one JSON
line: the preview's size and device time; the DSM's size, device time (into one device tensor), Gpx/s and the share of the
write floor (4 bytes per pixel at 6.29 TB/s, MI355X_MICROARCH.md); the CPU route on one band of 32 rows, its time and its
agreement with the device there.  Needs the GPU."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opencalibration_amd import capi, host, synth  # noqa: E402

WRITE_BPS = 6.29e12


def main():
    import torch

    torch.cuda.init()  # torch's HIP runtime comes up before libochip.so is loaded (as in bench.py)
    grid = synth.make_grid(40, 25, feats=16)
    pos = np.ascontiguousarray(grid.position, np.float64)
    rng = np.random.default_rng(0)
    surface = host.rebuild_mesh(pos)
    v = surface.arrays()["vertices"]
    surface.set_heights(v[:, 2] - grid.meta.get("height", 100.0) + rng.uniform(-2, 2, len(v)))
    n_tris = len(surface.arrays()["edges"])
    g = host.Graph()
    m = g.add_model(np.asarray(grid.model, np.float64))
    for p in pos:
        g.add_image(np.zeros((0, 2)), np.zeros(0, np.float32), np.zeros((0, 8), np.uint64), 0, m, p)
    g.set_orientations(np.ascontiguousarray(grid.orientation, np.float64))
    cols, rows = int(grid.model[8]) // 8, int(grid.model[9]) // 8
    for i in range(len(pos)):
        g.set_thumbnail(i, rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8))
    ctx = capi.Context(0)
    out = dict(images=len(pos), mesh_vertices=len(v), mesh_edges=n_tris, device=ctx.device_info()["name"])

    host.orthomosaic_thumbnail(g, [surface], ctx=ctx)  # warm-up (code objects, pool)
    t0 = time.perf_counter()
    th = host.orthomosaic_thumbnail(g, [surface], ctx=ctx)
    out.update(thumbnail_width=th["width"], thumbnail_height=th["height"], thumbnail_s=time.perf_counter() - t0,
               thumbnail_lit=float((th["rgba"][..., 3] == 255).mean()))

    plan = host.dsm_plan(g, [surface])
    W, H = plan["width"], plan["height"]
    mesh = host.OrthoMesh(ctx, [surface])
    dsm = torch.empty((H, W), dtype=torch.float32, device="cuda:0")
    host.dsm_render(plan, mesh=mesh, row0=0, rows=64, out=dsm[:64])  # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        host.dsm_render(plan, mesh=mesh, out=dsm)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    t = min(times)
    px = W * H
    out.update(dsm_width=W, dsm_height=H, dsm_gpx=px / 1e9, dsm_gsd=plan["gsd"], dsm_s=t, dsm_s_all=times,
               dsm_gpx_per_s=px / t / 1e9, dsm_write_floor_fraction=(4 * px / WRITE_BPS) / t,
               dsm_hit_fraction=float(1 - torch.isnan(dsm).float().mean().item()))
    del dsm

    r0, n = H // 2, 32
    t0 = time.perf_counter()
    cpu32, cpu_tri, cpu64, capped = host.dsm_render(plan, [surface], row0=r0, rows=n, debug=True)
    cpu_s = time.perf_counter() - t0
    dev32, dev_tri, dev64, _ = host.dsm_render(plan, [surface], mesh=mesh, row0=r0, rows=n, debug=True)
    same = dev_tri == cpu_tri
    other = ~same
    tol_ok = bool(np.all(np.abs(dev64[other] - cpu64[other]) <= 1e-9 * (1 + np.abs(cpu64[other]))))
    out.update(cpu_band_rows=n, cpu_band_px=n * W, cpu_band_s=cpu_s, cpu_threads=os.environ.get("OMP_NUM_THREADS"),
               device_band_s_equiv=t * n / H, cpu_over_device=cpu_s / (t * n / H),
               band_nan_masks_equal=bool(np.array_equal(np.isnan(cpu64), np.isnan(dev64))),
               band_same_triangle_bit_equal=bool(np.array_equal(dev64[same], cpu64[same], equal_nan=True)),
               band_pixels_other_triangle=int(other.sum()), band_other_triangle_within_tol=tol_ok,
               band_cpu_capped_walks=int(capped))
    mesh.close()
    g.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

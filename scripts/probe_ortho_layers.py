"""The layered full-resolution orthomosaic on C3 geometry: the cameras of synth.make_grid(40, 25), the mesh rebuilt under
them (rebuildMesh) with perturbed heights, the 1 000 views rendered into HBM (synth_views), the whole raster rendered in
bands of one 1 024-row tile row into device tensors.  Prints one JSON line: the raster and band count, the device time
(warm, best of 3, synchronised), Gpx/s per layer-pixel, the correspondence count, and the CPU route on one band of 64
rows at tile_size 64 with its exact agreement with the device there.  Needs the GPU."""
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
    quick = "--quick" in sys.argv  # the kernel-trace run: one pass over the raster
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
    cfg = host.LAYERS_CONFIG
    T, L = cfg["tile_size"], cfg["num_layers"]
    out = dict(images=len(pos), image_size=[W_img, H_img], device=ctx.device_info()["name"], width=W, height=H,
               layers=L, tile_size=T, bands=-(-H // T), gsd=plan["gsd"])
    mesh = host.OrthoMesh(ctx, [surface])
    bufs = dict(bgra=torch.empty((L, T, W, 4), dtype=torch.uint8, device="cuda:0"),
                camera_id=torch.empty((L, T, W), dtype=torch.int64, device="cuda:0"),
                weight=torch.empty((L, T, W), dtype=torch.float32, device="cuda:0"))

    def band_out(rows):  # contiguous (L, rows, ...) views of the band buffers
        return {k: t.view(-1)[:t[:, :rows].numel()].view(t[:, :rows].shape) for k, t in bufs.items()}

    def render_all():
        n_corr = 0
        for row0 in range(0, H, T):
            rows = min(T, H - row0)
            r = host.ortho_layers(plan, g, [surface], ptrs, mesh=mesh, row0=row0, tile_rows=1, out=band_out(rows))
            n_corr += len(r["correspondences"])
        torch.cuda.synchronize()
        return n_corr

    host.ortho_layers(plan, g, [surface], ptrs, mesh=mesh, row0=0, tile_rows=1, out=band_out(min(T, H)))  # warm-up
    times = []
    for _ in range(1 if quick else 3):
        t0 = time.perf_counter()
        n_corr = render_all()
        times.append(time.perf_counter() - t0)
    t = min(times)
    px = W * H
    out.update(device_s=t, device_s_all=times, gpx=px / 1e9, layer_gpx_per_s=px * L / t / 1e9, correspondences=n_corr,
               band_last_valid_fraction=[float((bufs["bgra"][k, ..., 3] == 255).float().mean().item()) for k in range(L)])
    if not quick:
        # one band of 64 rows at tile_size 64 by both routes.  The CPU route reads back the views the device's band used;
        # every other camera gets one shared zero image (a camera the device did not use would show as a difference)
        small = dict(cfg, tile_size=64)
        r0 = (H // 2) // 64 * 64
        t0 = time.perf_counter()
        dev = host.ortho_layers(plan, g, [surface], ptrs, mesh=mesh, row0=r0, tile_rows=1, config=small)
        dev_s = time.perf_counter() - t0
        used = set(int(v) for v in np.unique(dev["camera_id"]))
        node_ids = host.ortho_layers_cameras(g, [surface])["node_ids"]
        zero = np.zeros((H_img, W_img, 3), np.uint8)
        imgs = [ctx.synth_views_read(views, i, W_img, H_img) if int(n) in used else zero for i, n in enumerate(node_ids)]
        out.update(band_cameras_used=len(used - {0}))
        dsm = host.dsm_render(plan, [surface], mesh=mesh, row0=r0, rows=dev["rows"])
        t0 = time.perf_counter()
        cpu = host.ortho_layers(plan, g, [surface], imgs, row0=r0, tile_rows=1, config=small, dsm=dsm)
        cpu_s = time.perf_counter() - t0
        out.update(cpu_band_rows=dev["rows"], cpu_band_px=dev["rows"] * W, cpu_band_s=cpu_s, device_band_s=dev_s,
                   cpu_threads=os.environ.get("OMP_NUM_THREADS"),
                   band_bgra_equal=bool(np.array_equal(dev["bgra"], cpu["bgra"])),
                   band_ids_equal=bool(np.array_equal(dev["camera_id"], cpu["camera_id"])),
                   band_weights_equal=bool(np.array_equal(dev["weight"].view(np.uint32), cpu["weight"].view(np.uint32))),
                   band_correspondences=len(cpu["correspondences"]),
                   band_correspondences_equal=dev["correspondences"].tobytes() == cpu["correspondences"].tobytes())
    mesh.close()
    ctx.synth_views_free(views)
    g.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

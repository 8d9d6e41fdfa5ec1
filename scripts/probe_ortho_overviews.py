"""The averaged overview levels on C3 geometry: the scene of probe_ortho_blend.py - the cameras of
synth.make_grid(40, 25), the rebuilt and perturbed mesh, the 1 000 views rendered into HBM, 2 layers, bands of one
1 024-row tile row.  Prints one JSON line: ortho_mosaic end to end without and with overviews=True, alternating in one
process, three runs each (the run without is the unchanged path and the yardstick; the verdict is "within 2 %" unless the
yardstick's own spread is wider, then the spread is reported instead); the overview pass alone over the finished mosaic
and DSM in bands of 1 024 rows (best of 3, feeds and finish, levels allocated before the clock) with the bytes it moves;
the fused route against the one-level route (OCHIP_TEST_HOOKS=overview_per_level, read on every call) on the whole
raster, and the device against the CPU route on the first 4 096 rows, both bit for bit.  --quick: one ortho_mosaic pass
with overviews (the kernel-trace run).  Needs the GPU."""
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
    T = host.BLEND_CONFIG["tile_size"]
    node_ids = host.ortho_layers_cameras(g, [surface])["node_ids"]
    crng = np.random.default_rng(1)
    cb = dict(per_image={int(n): dict(lab_offset=crng.normal(0, 2, 3), brdf=0.5, slope=crng.normal(0, 1, 2))
                         for n in node_ids[::2]}, per_model={0: (3.0, -1.0, 0.5)})
    sizes = host.overview_levels(W, H)
    out = dict(images=len(pos), device=ctx.device_info()["name"], width=W, height=H, tile_size=T, bands=-(-H // T),
               gpx=W * H / 1e9, levels=len(sizes), smallest_level=list(sizes[-1]))
    mesh = host.OrthoMesh(ctx, [surface])
    dev = "cuda:0"
    mosaic = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)

    def end_to_end(overviews):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = host.ortho_mosaic(plan, g, [surface], ptrs, mesh=mesh, color_balance=cb, out=mosaic, overviews=overviews)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    if quick:
        out.update(mosaic_overviews_s=end_to_end(True)[0])
    else:
        end_to_end(True)  # warms the pools and the allocator for both
        plain, over = [], []
        for _ in range(3):
            plain.append(end_to_end(False)[0])
            s, (_, levels) = end_to_end(True)
            over.append(s)
        spread = (max(plain) - min(plain)) / min(plain)
        excess = min(over) / min(plain) - 1.0
        out.update(mosaic_s_all=plain, mosaic_overviews_s_all=over, mosaic_s=min(plain), mosaic_overviews_s=min(over),
                   yardstick_spread=spread, overviews_excess=excess,
                   verdict=("yardstick spread wider than 2 %" if spread > 0.02 else
                            "within 2 %" if excess <= 0.02 else "exceeds 2 %"))
        # the pass alone over the finished rasters, band by band as the mosaic feeds it
        dsm = torch.empty((H, W), dtype=torch.float32, device=dev)
        host.dsm_render(plan, [surface], mesh=mesh, out=dsm)
        tail = {host.OVERVIEW_RGBA8: (4,), host.OVERVIEW_FLOAT32: ()}
        dtype = {host.OVERVIEW_RGBA8: torch.uint8, host.OVERVIEW_FLOAT32: torch.float32}
        bufs = {k: [torch.empty(s + tail[k], dtype=dtype[k], device=dev) for s in sizes] for k in tail}

        def pass_alone():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for kind, raster in ((host.OVERVIEW_RGBA8, mosaic), (host.OVERVIEW_FLOAT32, dsm)):
                with host.OrthoOverviews(kind, W, H, ctx=ctx, on_device=True, levels=bufs[kind]) as b:
                    for row0 in range(0, H, T):
                        b.feed(row0, raster[row0:row0 + T])
                    b.finish()
            return time.perf_counter() - t0

        alone = [pass_alone() for _ in range(3)]
        # level 0 read once, every level written once, levels 6 .. read once more by the one-level kernel (negligible)
        moved = 2 * 4 * (W * H + sum(r * c for r, c in sizes))
        out.update(pass_s_all=alone, pass_s=min(alone), pass_bytes=moved, pass_tb_per_s=moved / min(alone) / 1e12)
        fused = [[l.clone() for l in bufs[k]] for k in tail]
        os.environ["OCHIP_TEST_HOOKS"] = "overview_per_level"
        per_level = [pass_alone() for _ in range(2)]
        del os.environ["OCHIP_TEST_HOOKS"]
        out.update(per_level_pass_s=min(per_level),
                   routes_equal=all(torch.equal(a.view(torch.uint8), b.view(torch.uint8))
                                    for f, k in zip(fused, tail) for a, b in zip(f, bufs[k])),
                   mosaic_levels_equal=all(torch.equal(a, b) for a, b in zip(levels["rgba"], fused[0])))
        rows = min(H, 4096)
        crop, zcrop = mosaic[:rows].contiguous(), dsm[:rows].contiguous()
        t0 = time.perf_counter()
        c_rgba, c_dsm = host.ortho_overviews(crop.cpu().numpy()), host.ortho_overviews(zcrop.cpu().numpy())
        cpu_s = time.perf_counter() - t0
        d_rgba, d_dsm = host.ortho_overviews(crop, ctx), host.ortho_overviews(zcrop, ctx)
        out.update(cpu_crop_rows=rows, cpu_crop_s=cpu_s, cpu_threads=os.environ.get("OMP_NUM_THREADS"),
                   cpu_equal=all(np.array_equal(a.cpu().numpy().view(np.uint8), b.view(np.uint8))
                                 for a, b in zip(d_rgba + d_dsm, c_rgba + c_dsm)),
                   opaque_fraction=float((mosaic[..., 3] == 255).float().mean().item()),
                   dsm_nan_fraction=float(torch.isnan(dsm).float().mean().item()))
    mesh.close()
    ctx.synth_views_free(views)
    g.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""The scenarios of test_gpu_ortho_blend.py, run in a child process (as layers_gpu_child.py, torch first): the device
route of the blend against the CPU route, bit for bit.  `python blend_gpu_child.py <tests dir> <repo dir>` runs every
scenario and prints one JSON line {scenario: "ok" or the failure's traceback}."""
import json
import sys
import traceback

import numpy as np
import torch

torch.cuda.init()
if __name__ == "__main__":
    sys.path[:0] = sys.argv[1:3]

from layers_fixtures import four_camera_scene, noise_images  # noqa: E402
from ortho_fixtures import cloud_surface, jittered_cameras, make_graph, perturbed_mesh, three_cameras  # noqa: E402
from opencalibration_amd import capi, host  # noqa: E402


def small_plan(gsd=0.05):
    return dict(width=int(10.5 / gsd), height=int(9.0 / gsd), gsd=gsd, min_x=-2.0, max_x=8.5, min_y=-2.0, max_y=7.0,
                mean_camera_z=10.0)


def color_table(g, surfaces, seed, model0=True):
    cams = host.ortho_layers_cameras(g, surfaces)
    rng = np.random.default_rng(seed)
    per_image = {int(n): dict(lab_offset=rng.normal(0, 4, 3), brdf=float(rng.normal(0, 2)), slope=rng.normal(0, 3, 2))
                 for n in cams["node_ids"][::2]}
    per_model = {5: (40.0, -3.0, 1.0)}
    if model0:
        per_model[0] = tuple(rng.normal(0, 5, 3))
    return dict(per_image=per_image, per_model=per_model)


def same_f32(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def layers_cfg(config):
    return {k: v for k, v in config.items() if k in host.LAYERS_CONFIG}


def compare(ctx, g, surfaces, images, plan, config, color_balance=None, row0=0, tile_rows=None, edit=None):
    """one band: layers and DSM on the device, then the blend on both routes from the same inputs (edit(layers): a change
    to the layers first, which also leaves the weight cross-check out)"""
    dimg = [torch.from_numpy(im).to("cuda:0") for im in images]
    with host.OrthoMesh(ctx, surfaces) as mesh:
        lay = host.ortho_layers(plan, g, surfaces, dimg, mesh=mesh, row0=row0, tile_rows=tile_rows,
                                config=layers_cfg(config))
        dsm = host.dsm_render(plan, surfaces, mesh=mesh, row0=row0, rows=lay["rows"])
    if edit is not None:
        edit(lay)
    dev, ddbg = host.ortho_blend(plan, g, surfaces, lay, dsm, color_balance, ctx=ctx, config=config, debug=True)
    cpu, cdbg = host.ortho_blend(plan, g, surfaces, lay, dsm, color_balance, config=config, debug=True)
    assert np.array_equal(dev, cpu), int((dev != cpu).any(-1).sum())
    for k in ("weight", "dist", "lab"):
        assert same_f32(ddbg[k], cdbg[k]), k
    # the recomputed weights are the layer pass's (same heights, same cameras)
    assert edit is not None or same_f32(ddbg["weight"], lay["weight"]), int((ddbg["weight"] != lay["weight"]).sum())
    again = host.ortho_blend(plan, g, surfaces, lay, dsm, color_balance, ctx=ctx, config=config)
    assert np.array_equal(again, dev)
    return dev, ddbg, lay, dsm


def scenario_three_camera_fixture(ctx):
    pos, ori, model, _ = three_cameras()
    g = make_graph(pos, ori, model)
    pts = cloud_surface([(5, 5, -10), (10, 10, -5), (5, 10, -7.5), (10, 5, -8)])
    s = host.rebuild_mesh(np.array(pos, np.float64), previous=pts)
    plan = host.dsm_plan(g, [s], max_output_megapixels=0.05)
    imgs = noise_images(3, 600, 800, 1)
    cfg = dict(tile_size=64, blend_transition_radius=8)
    for cb in (None, color_table(g, [s], 1), color_table(g, [s], 2, model0=False)):
        rgba, dbg, _, _ = compare(ctx, g, [s], imgs, plan, cfg, cb)
    assert (rgba[..., 3] == 255).any() and (rgba[..., 3] == 0).any()
    g.close()


def scenario_distorted_tiles_and_bands(ctx):
    g, s, imgs = four_camera_scene()
    plan = small_plan()
    cfg = dict(tile_size=64, blend_transition_radius=16)
    cb = color_table(g, [s], 3)
    whole, dbg, lay, dsm = compare(ctx, g, [s], imgs, plan, cfg, cb)
    assert plan["height"] % 64 and plan["width"] % 64
    d = dbg["dist"]
    # some tile without a boundary (+inf) and some tile without a valid pixel (the checkerboard)
    tiles_inf = [np.isinf(d[r:r + 64, c:c + 64]).all() for r in range(0, d.shape[0], 64) for c in range(0, d.shape[1], 64)]
    assert any(tiles_inf) and (d == 0).any()

    def hole(lay):  # a tile with no valid pixel, and one whose layer 0 is one camera (no boundary)
        lay["bgra"][:, 64:128, 0:64, 3] = 0
        lay["camera_id"][0, 0:64, 64:128] = lay["camera_id"][0, 0, 64]
        lay["bgra"][0, 0:64, 64:128, 3] = 255

    holed, hdbg, _, _ = compare(ctx, g, [s], imgs, plan, cfg, cb, edit=hole)
    assert (holed[64:128, 0:64, 3] == 0).all() and np.isinf(hdbg["dist"][0:64, 64:128]).all()
    # bands of one tile row equal the single call
    for row0 in range(0, plan["height"], 64):
        band = dict(bgra=lay["bgra"][:, row0:row0 + 64], camera_id=lay["camera_id"][:, row0:row0 + 64], row0=row0)
        got = host.ortho_blend(plan, g, [s], band, dsm[row0:row0 + 64], cb, ctx=ctx, config=cfg)
        assert np.array_equal(got, whole[row0:row0 + 64]), row0
    g.close()


def scenario_partial_tiles_width_1_to_3(ctx):
    g, s, imgs = four_camera_scene(seed=1)
    for extra in (1, 2, 3):
        plan = small_plan(0.1)
        plan["width"], plan["height"] = 64 + extra, 64 + extra
        compare(ctx, g, [s], imgs, plan, dict(tile_size=64, blend_transition_radius=8), color_table(g, [s], extra))
    g.close()


def scenario_perturbed_mesh_layers(ctx, num_layers):
    pos, ori = jittered_cameras(3, 3, spacing=8.0, height=40.0, seed=3)
    model = [200, 100, 75, -0.03, 0.002, 0, 0.0005, 0.0003, 200, 150]
    g = make_graph(pos, ori, model)
    s = perturbed_mesh(pos, seed=4)
    b = host.ortho_bounds([s])
    plan = dict(width=180, height=150, gsd=0.12, min_x=b["min_x"] + 4, max_x=b["min_x"] + 4 + 180 * 0.12,
                min_y=b["max_y"] - 4 - 150 * 0.12, max_y=b["max_y"] - 4, mean_camera_z=40.0)
    compare(ctx, g, [s], noise_images(9, 150, 200, 5), plan, dict(num_layers=num_layers, tile_size=64), color_table(g, [s], 4))
    g.close()


def scenario_two_surfaces(ctx):
    g, s, imgs = four_camera_scene(seed=2)
    s2 = host.rebuild_mesh(np.array([(0, 0, 10), (6, 0.3, 10), (0.2, 5, 10.5)], np.float64),
                           previous=cloud_surface([(-6, -6, 1), (12, -6, 1), (12, 11, 1), (-6, 11, 1)]))
    compare(ctx, g, [s, s2], imgs, small_plan(0.08), dict(tile_size=32), color_table(g, [s, s2], 5))
    g.close()


def scenario_device_tensor_mosaic(ctx):
    g, s, imgs = four_camera_scene(seed=4)
    plan = small_plan(0.1)
    cfg = dict(tile_size=32, blend_transition_radius=10)
    cb = color_table(g, [s], 6)
    with host.OrthoMesh(ctx, [s]) as mesh:
        out = torch.full((plan["height"], plan["width"], 4), 7, dtype=torch.uint8, device="cuda:0")
        dev = host.ortho_mosaic(plan, g, [s], [torch.from_numpy(im).to("cuda:0") for im in imgs], mesh=mesh, config=cfg,
                                color_balance=cb, tile_rows=2, out=out)
        assert dev is out
        dsm = host.dsm_render(plan, [s], mesh=mesh)
    # the CPU route on the device's heights, band by band
    cpu = np.zeros((plan["height"], plan["width"], 4), np.uint8)
    for row0 in range(0, plan["height"], 64):
        rows = min(64, plan["height"] - row0)
        lay = host.ortho_layers(plan, g, [s], imgs, row0=row0, tile_rows=2, config=layers_cfg(cfg),
                                dsm=dsm[row0:row0 + rows])
        host.ortho_blend(plan, g, [s], lay, dsm[row0:row0 + rows], cb, config=cfg, out=cpu[row0:row0 + rows])
    assert np.array_equal(out.cpu().numpy(), cpu)
    g.close()


def scenario_laplacian_blend_random(ctx):
    rng = np.random.default_rng(7)
    for size in list(range(1, 20)) + [31, 32, 33, 47, 64, 65, 70]:
        for nl in (1, 3):
            h = size if size % 3 else max(1, size - 5)
            lab = np.stack([rng.uniform(0, 100, (nl, h, size)), rng.uniform(-127, 127, (nl, h, size)),
                            rng.uniform(-127, 127, (nl, h, size))], -1).astype(np.float32)
            w = (rng.uniform(0, 1, (nl, h, size)) * (rng.uniform(size=(nl, h, size)) > 0.3)).astype(np.float32)
            for levels in (1, 4, 9):
                dev = host.laplacian_blend(lab, w, levels, ctx=ctx)
                cpu = host.laplacian_blend(lab, w, levels)
                assert np.array_equal(dev, cpu), (size, nl, levels)


SCENARIOS = {
    "three_camera_fixture_color_tables": scenario_three_camera_fixture,
    "distorted_scene_tiles_and_bands": scenario_distorted_tiles_and_bands,
    "partial_tiles_width_1_to_3": scenario_partial_tiles_width_1_to_3,
    "perturbed_mesh_layers_1": lambda ctx: scenario_perturbed_mesh_layers(ctx, 1),
    "perturbed_mesh_layers_3": lambda ctx: scenario_perturbed_mesh_layers(ctx, 3),
    "two_surfaces": scenario_two_surfaces,
    "device_tensor_mosaic": scenario_device_tensor_mosaic,
    "laplacian_blend_random_sizes": scenario_laplacian_blend_random,
}

if __name__ == "__main__":
    ctx = capi.Context(0)
    res = {}
    for name, fn in SCENARIOS.items():
        try:
            fn(ctx)
            res[name] = "ok"
        except Exception:
            res[name] = traceback.format_exc()
    ctx.close()
    print(json.dumps(res))

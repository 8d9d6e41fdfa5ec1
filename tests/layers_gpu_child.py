"""The scenarios of test_gpu_ortho_layers.py, run in a child process: torch has to bring up its HIP runtime before
libochip.so is loaded (as bench.py does), which a pytest process that ran other device tests first cannot arrange, and the
device route reads its images from torch tensors.  `python layers_gpu_child.py <tests dir> <repo dir>` runs every
scenario and prints one JSON line {scenario: "ok" or the failure's traceback}."""
import json
import sys
import traceback

import numpy as np
import torch

torch.cuda.init()
if __name__ == "__main__":
    sys.path[:0] = sys.argv[1:3]

from layers_fixtures import DISTORTED, expected_layers, knn_agrees, four_camera_scene, noise_images, plan_with_gsd  # noqa: E402
from ortho_fixtures import (cloud_surface, functional_scene, jittered_cameras, make_graph, perturbed_mesh,  # noqa: E402
                            three_cameras)
from ortho_stream_fixtures import BAND_SET_SCENES, knn_band_sets, scene_knn_overflow  # noqa: E402
from opencalibration_amd import capi, host  # noqa: E402


def dev_images(images):
    return [torch.from_numpy(im).to("cuda:0") for im in images]


def assert_same(dev, cpu):
    assert np.array_equal(dev["bgra"], cpu["bgra"])
    assert np.array_equal(dev["camera_id"], cpu["camera_id"])
    assert np.array_equal(dev["weight"].view(np.uint32), cpu["weight"].view(np.uint32))
    assert len(dev["correspondences"]) == len(cpu["correspondences"])
    assert dev["correspondences"].tobytes() == cpu["correspondences"].tobytes()


def compare(ctx, g, surfaces, images, plan, config=None, row0=0, tile_rows=None, knn=False):
    """device band vs the CPU route on the device's own heights (the DSM kernel's)"""
    with host.OrthoMesh(ctx, surfaces) as mesh:
        dev = host.ortho_layers(plan, g, surfaces, dev_images(images), mesh=mesh, row0=row0, tile_rows=tile_rows, config=config,
                                debug_knn=knn)
        dsm = host.dsm_render(plan, surfaces, mesh=mesh, row0=row0, rows=dev["rows"])
    cpu = host.ortho_layers(plan, g, surfaces, images, row0=row0, tile_rows=tile_rows, config=config, dsm=dsm, debug_knn=knn)
    assert_same(dev, cpu)
    if knn:
        assert np.array_equal(dev["knn"], cpu["knn"])
    return dev, cpu, dsm


def small_plan(gsd=0.05):
    return dict(width=int(10.5 / gsd), height=int(9.0 / gsd), gsd=gsd, min_x=-2.0, max_x=8.5, min_y=-2.0, max_y=7.0,
                mean_camera_z=10.0)


def scenario_three_camera_fixture_and_functional_scene(ctx):
    pos, ori, model, _ = three_cameras()
    g = make_graph(pos, ori, model)
    pts = cloud_surface([(5, 5, -10), (10, 10, -5), (5, 10, -7.5), (10, 5, -8)])
    s = host.rebuild_mesh(np.array(pos, np.float64), previous=pts)
    plan = host.dsm_plan(g, [s], max_output_megapixels=0.05)
    dev, _, _ = compare(ctx, g, [s], noise_images(3, 600, 800, 1), plan, config=dict(tile_size=64, correspondence_subsample=7))
    assert (dev["bgra"][0, ..., 3] == 255).any()
    g.close()
    g, s = functional_scene()
    plan = host.dsm_plan(g, [s])
    dev, _, _ = compare(ctx, g, [s], noise_images(2, 100, 100, 2), plan, config=dict(num_layers=2, correspondence_subsample=5))
    assert (dev["bgra"][0, ..., 3] == 255).any()  # two footprints that do not overlap: one layer
    g.close()


def scenario_distorted_scene_tiles_bands_and_knn(ctx):
    g, s, imgs = four_camera_scene()
    plan = small_plan()
    cfg = dict(tile_size=64, correspondence_subsample=9)
    whole, cpu, dsm = compare(ctx, g, [s], imgs, plan, config=cfg, knn=True)
    assert plan["height"] % 64 and plan["width"] % 64  # partial last tiles
    cams = host.ortho_layers_cameras(g, [s])
    pos = cams["cams"][:, :3]
    ori = g.orientations()
    knn, layers = expected_layers(plan, cams["cams"], ori, pos, [DISTORTED] * 4, dsm, 2, order_in=whole["knn"])
    assert knn_agrees(whole["knn"], knn, plan, cams["cams"])
    idx = {int(n): i for i, n in enumerate(cams["node_ids"])}
    got = np.vectorize(lambda v: idx.get(int(v), -1))(whole["camera_id"])
    assert np.array_equal(got, layers)
    # bands of one tile row each equal the single call
    with host.OrthoMesh(ctx, [s]) as mesh:
        bands = list(host.ortho_layers_bands(plan, g, [s], dev_images(imgs), mesh=mesh, tile_rows=1, config=cfg))
    assert np.array_equal(np.concatenate([b["bgra"] for b in bands], axis=1), whole["bgra"])
    assert np.array_equal(np.concatenate([b["camera_id"] for b in bands], axis=1), whole["camera_id"])
    assert np.concatenate([b["correspondences"] for b in bands]).tobytes() == whole["correspondences"].tobytes()
    g.close()


def scenario_perturbed_refined_mesh_layers(ctx, num_layers):
    pos, ori = jittered_cameras(3, 3, spacing=8.0, height=40.0, seed=3)
    model = [200, 100, 75, -0.03, 0.002, 0, 0.0005, 0.0003, 200, 150]
    g = make_graph(pos, ori, model)
    s = perturbed_mesh(pos, seed=4)
    b = host.ortho_bounds([s])
    plan = dict(width=180, height=150, gsd=0.12, min_x=b["min_x"] + 4, max_x=b["min_x"] + 4 + 180 * 0.12,
                min_y=b["max_y"] - 4 - 150 * 0.12, max_y=b["max_y"] - 4, mean_camera_z=40.0)
    dev, _, _ = compare(ctx, g, [s], noise_images(9, 150, 200, 5), plan,
                        config=dict(num_layers=num_layers, tile_size=64, correspondence_subsample=6))
    valid = dev["bgra"][..., 3] == 255
    assert valid[num_layers - 1].any()
    assert not (valid[1:] & ~valid[:-1]).any()
    assert (len(dev["correspondences"]) > 0) == (num_layers > 1)
    g.close()


def scenario_two_surfaces(ctx):
    g, s, imgs = four_camera_scene(seed=2)
    s2 = host.rebuild_mesh(np.array([(0, 0, 10), (6, 0.3, 10), (0.2, 5, 10.5)], np.float64),
                           previous=cloud_surface([(-6, -6, 1), (12, -6, 1), (12, 11, 1), (-6, 11, 1)]))
    compare(ctx, g, [s, s2], imgs, small_plan(0.08), config=dict(tile_size=32, correspondence_subsample=4))
    g.close()


def scenario_single_pixel_path_and_radius_cap(ctx):
    g, s, imgs = four_camera_scene(seed=3)
    small, _, _ = compare(ctx, g, [s], imgs, plan_with_gsd(small_plan(), 0.04), config=dict(tile_size=128))
    big, _, _ = compare(ctx, g, [s], imgs, plan_with_gsd(small_plan(), 2.5), config=dict(correspondence_subsample=1))
    assert (small["bgra"][..., 3] == 255).any() and (big["bgra"][..., 3] == 255).any()
    g.close()


def scenario_device_tensor_outputs(ctx):
    g, s, imgs = four_camera_scene(seed=4)
    plan = small_plan(0.1)
    cfg = dict(tile_size=32, correspondence_subsample=5)
    L, rows, w = 2, plan["height"], plan["width"]
    out = dict(bgra=torch.full((L, rows, w, 4), 7, dtype=torch.uint8, device="cuda:0"),
               camera_id=torch.full((L, rows, w), 7, dtype=torch.int64, device="cuda:0"),
               weight=torch.full((L, rows, w), 7.0, dtype=torch.float32, device="cuda:0"))
    with host.OrthoMesh(ctx, [s]) as mesh:
        dev = host.ortho_layers(plan, g, [s], dev_images(imgs), mesh=mesh, config=cfg, out=out)
        dsm = host.dsm_render(plan, [s], mesh=mesh)
    cpu = host.ortho_layers(plan, g, [s], imgs, config=cfg, dsm=dsm)
    res = dict(bgra=out["bgra"].cpu().numpy(), camera_id=out["camera_id"].cpu().numpy().view(np.uint64),
               weight=out["weight"].cpu().numpy(), correspondences=dev["correspondences"])
    assert_same(res, cpu)
    g.close()


def scenario_knn_on_band_set_scenes(ctx):
    """pass 1's search and the band kernel's copy of it agree: the render's own kNN lists give the band kernel's sets"""
    for name, scene in BAND_SET_SCENES.items():
        g, s, imgs, plan, cfg = scene()
        dev, _, _ = compare(ctx, g, [s], imgs, plan, config=cfg, knn=True)
        sets = host.ortho_band_cameras(plan, g, [s], tile_rows=1, config=cfg, ctx=ctx)
        assert np.array_equal(knn_band_sets(dev["knn"], len(imgs), cfg["tile_size"]), sets), name
        g.close()


def scenario_knn_candidate_overflow(ctx):
    g, s, imgs, plan, cfg = scene_knn_overflow()
    dev, _, _ = compare(ctx, g, [s], imgs, plan, config=cfg, knn=True)
    assert (dev["bgra"][0, ..., 3] == 255).any()
    g.close()


SCENARIOS = {
    "three_camera_fixture_and_functional_scene": scenario_three_camera_fixture_and_functional_scene,
    "distorted_scene_tiles_bands_and_knn": scenario_distorted_scene_tiles_bands_and_knn,
    "perturbed_refined_mesh_layers_1": lambda ctx: scenario_perturbed_refined_mesh_layers(ctx, 1),
    "perturbed_refined_mesh_layers_3": lambda ctx: scenario_perturbed_refined_mesh_layers(ctx, 3),
    "two_surfaces": scenario_two_surfaces,
    "single_pixel_path_and_radius_cap": scenario_single_pixel_path_and_radius_cap,
    "device_tensor_outputs": scenario_device_tensor_outputs,
    "knn_on_band_set_scenes": scenario_knn_on_band_set_scenes,
    "knn_candidate_overflow": scenario_knn_candidate_overflow,
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

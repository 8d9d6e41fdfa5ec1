"""The orthomosaic preview and DSM raster on the host: the reference's known answers of test/test_ortho.cpp restated
with their values and tolerances (bounds, GSD, context, rayTraceHeight, the functional scene on the CPU route), the CPU
route's heights against a brute-force evaluation of the mesh, and the two output clamps.  No device."""
import numpy as np
import pytest

from ortho_fixtures import (brute_force_heights, cloud_surface, functional_scene, jittered_cameras, make_graph,
                            perturbed_mesh, pixel_centres, plan_over, project, three_cameras)
from opencalibration_amd import capi, host


def test_calculate_bounds_cloud():                                         # test_ortho.cpp:109-127
    b = host.ortho_bounds([cloud_surface([(0, 0, 10), (10, 20, 30)])])
    assert (b["min_x"], b["max_x"], b["min_y"], b["max_y"], b["mean_surface_z"]) == (0, 10, 0, 20, 20)


def test_calculate_bounds_mesh():                                          # test_ortho.cpp:129-150
    s = host.Surface().set(np.array([(1, 2, 3), (5, 6, 7)], np.float64), np.zeros((0, 5), np.uint64))
    b = host.ortho_bounds([s])
    assert (b["min_x"], b["max_x"], b["min_y"], b["max_y"], b["mean_surface_z"]) == (1, 5, 2, 6, 5)


def test_mesh_hides_clouds_in_bounds():
    """A surface's clouds count only when it has no mesh (ortho.cpp:305-320)."""
    s = host.Surface().set(np.array([(1, 2, 3), (5, 6, 7)], np.float64), np.zeros((0, 5), np.uint64),
                           cloud=np.array([(-100, -100, 1000)], np.float64))
    assert host.ortho_bounds([s])["min_x"] == 1


def test_calculate_gsd():                                                  # test_ortho.cpp:152-178
    pos, ori, model, thumbs = three_cameras()
    g = make_graph(pos[:1], ori[:1], model, thumbs[:1])
    assert host.ortho_gsd(g, g.node_ids, 0) == pytest.approx(0.09, abs=1e-7)
    g.close()


def test_calculate_gsd_multi():                                            # test_ortho.cpp:258-288
    pos, ori, model, thumbs = three_cameras()
    g = make_graph([pos[0], (11, 9, 19)], ori[:2], model, thumbs[:2])
    assert host.ortho_gsd(g, g.node_ids, 0) == pytest.approx(0.14, abs=1e-7)
    g.close()


def test_prepare_context():                                                # test_ortho.cpp:180-218
    pos, ori, model, thumbs = three_cameras()
    g = make_graph(pos, ori, model, thumbs)
    c = host.ortho_context(g, [cloud_surface([(5, 5, -10), (10, 10, -5)])])
    assert (c["min_x"], c["max_x"], c["min_y"], c["max_y"]) == (5, 10, 5, 10)
    assert c["mean_surface_z"] == -7.5
    assert c["involved"] == 3
    assert c["gsd"] > 0
    assert c["mean_camera_z"] == 9
    assert c["average_camera_elevation"] == 16.5
    g.close()


def test_involved_nodes_need_a_finite_orientation():
    pos, ori, model, thumbs = three_cameras()
    ori = np.array(ori)
    ori[1] = np.nan
    g = make_graph(pos, ori, model, thumbs)
    c = host.ortho_context(g, [cloud_surface([(5, 5, -10), (10, 10, -5)])])
    assert c["involved"] == 2 and c["mean_camera_z"] == 9
    g.close()


def test_ray_trace_height():                                               # test_ortho.cpp:220-238
    pts = cloud_surface([(5, 5, -10), (10, 10, -5), (5, 10, -7.5)])
    s = host.rebuild_mesh(np.array([(0, 0, 10), (10, 0, 10)], np.float64), previous=pts)
    z = host.ray_trace_height(7.5, 7.5, 10, [s])
    assert not np.isnan(z) and -10 < z < 0


def test_ray_trace_height_miss():                                          # test_ortho.cpp:240-256
    pts = cloud_surface([(5, 5, -10), (6, 5, -10), (5, 6, -10)])
    s = host.rebuild_mesh(np.array([(0, 0, 10)], np.float64), previous=pts)
    assert np.isnan(host.ray_trace_height(100, 100, 10, [s]))


def check_functional_scene(out, g):
    """The THEN of test_ortho.cpp:351-373: red with node 0's id at world (0, 0), blue with node 1's at (10, 0)."""
    gsd = out["gsd"]
    assert gsd > 0
    assert out["min_x"] == -20 and out["max_y"] == 20
    row_y0, col_x0, col_x10 = int(20 / gsd), int((0 + 20) / gsd), int((10 + 20) / gsd)
    rgba, ids = out["rgba"], out["ids"]
    assert tuple(rgba[row_y0, col_x0, :3]) == (255, 0, 0)
    assert ids[row_y0, col_x0] == g.node_ids[0] & 0xFFFFFFFF
    assert tuple(rgba[row_y0, col_x10, :3]) == (0, 0, 255)
    assert ids[row_y0, col_x10] == g.node_ids[1] & 0xFFFFFFFF


def test_functional_ortho_scene_cpu():                                     # test_ortho.cpp:290-374
    g, s = functional_scene()
    out = host.orthomosaic_thumbnail(g, [s])
    # 2 x 100 x 100 input pixels clamp the natural ~5 MP output (the reference's comment: GSD ~0.316, ~126 x 158)
    assert out["width"] * out["height"] <= 2 * 100 * 100
    check_functional_scene(out, g)
    g.close()


def test_thumbnail_pixel_classes_cpu():
    """Every pixel is a camera's colour (alpha 255, a node id), the checkerboard (alpha 0, grey 64 / 128 by parity,
    no id) or outside every surface ((0, 0, 0, 0), no id); the heights taken back in give the same raster."""
    g, s = functional_scene()
    out = host.orthomosaic_thumbnail(g, [s], want_z=True)
    rgba, ids, z = out["rgba"], out["ids"], out["z"]
    lit = rgba[..., 3] == 255
    assert set(np.unique(ids[lit]).tolist()) <= {i & 0xFFFFFFFF for i in g.node_ids} and lit.any()
    bg = ~lit & ~np.isnan(z)
    r, c = np.nonzero(bg)
    assert np.all(ids[bg] == 0xFFFFFFFF) and np.all(rgba[bg][:, 3] == 0)
    assert np.array_equal(rgba[bg][:, 0], np.where((r + c) % 2 == 0, 64, 128))
    miss = np.isnan(z)
    assert np.all(rgba[miss] == 0) and np.all(ids[miss] == 0xFFFFFFFF)
    again = host.orthomosaic_thumbnail(g, [s], z_in=z)
    assert np.array_equal(again["rgba"], rgba) and np.array_equal(again["ids"], ids)
    g.close()


def test_thumbnail_needs_thumbnails():
    pos, ori, model, thumbs = three_cameras()
    g = make_graph(pos, ori, model, thumbs[:2])
    with pytest.raises(capi.OchipError, match="thumbnail"):
        host.orthomosaic_thumbnail(g, [cloud_surface([(5, 5, -10), (10, 10, -5)])])
    g.close()


@pytest.mark.parametrize("seed", [1, 2])
def test_cpu_dsm_heights_against_brute_force(seed):
    """The CPU route's fp64 heights equal barycentric interpolation in a triangle holding the pixel centre (1e-9), on
    a rebuilt mesh with perturbed heights; NaN exactly off the mesh; no walk ran out of steps."""
    pos, _ = jittered_cameras(5, 4, seed=seed)
    s = perturbed_mesh(pos, seed=seed)
    plan = plan_over(s, 0.5)
    z32, tri, z64, capped = host.dsm_render(plan, [s], debug=True)
    assert capped == 0
    xs, ys = pixel_centres(plan)
    ref = brute_force_heights(s, xs, ys)
    assert np.array_equal(np.isnan(z64), np.isnan(ref))
    hit = ~np.isnan(ref)
    assert hit.mean() > 0.5 and (~hit).any()
    np.testing.assert_allclose(z64[hit], ref[hit], rtol=0, atol=1e-9 * (1 + np.abs(ref[hit])).max())
    assert np.array_equal(z32, z64.astype(np.float32), equal_nan=True)
    assert np.all((tri == 0xFFFFFFFF) == ~hit)


def test_cpu_dsm_bands_equal_whole():
    pos, _ = jittered_cameras(4, 3, seed=5)
    s = perturbed_mesh(pos, seed=5)
    plan = plan_over(s, 0.7)
    whole = host.dsm_render(plan, [s])
    parts = [host.dsm_render(plan, [s], row0=r, rows=min(17, plan["height"] - r)) for r in range(0, plan["height"], 17)]
    assert np.array_equal(np.concatenate(parts), whole, equal_nan=True)


def test_dsm_plan_and_megapixel_cap():
    """The DSM plan of the three-camera scene at full resolution, then under max_output_megapixels."""
    pos, ori, model, thumbs = three_cameras()
    g = make_graph(pos, ori, model)
    s = cloud_surface([(5, 5, -10), (10, 10, -5)])
    p = host.dsm_plan(g, [s])
    c = host.ortho_context(g, [s], thumbnail=False)
    assert p["gsd"] == c["gsd"] and p["mean_camera_z"] == 9
    assert p["width"] == int(5 / c["gsd"]) and p["height"] == int(5 / c["gsd"])
    q = host.dsm_plan(g, [s], max_output_megapixels=0.01)
    assert q["width"] * q["height"] <= 10000 and q["gsd"] > p["gsd"]
    g.close()


def test_clamp_output_resolution():
    """clampOutputResolution: above the input pixel count the GSD grows by sqrt(output / input) and the size shrinks by
    it, truncated; at or below it (or with no input) nothing changes."""
    gsd, w, h = host.ortho_clamp_resolution(10000, 0.02, 700, 200)
    f = np.sqrt(700 * 200 / 10000)
    assert gsd == 0.02 * f and (w, h) == (int(700 / f), int(200 / f))
    assert host.ortho_clamp_resolution(140000, 0.02, 700, 200) == (0.02, 700, 200)
    assert host.ortho_clamp_resolution(0, 0.02, 700, 200) == (0.02, 700, 200)


def test_clamp_output_megapixels():
    """clampOutputMegapixels: no cap for a non-finite or non-positive limit or a limit below one pixel; otherwise the
    same scaling with the size kept at >= 1."""
    gsd, w, h = host.ortho_clamp_megapixels(0.01, 0.5, 1000, 50)
    f = np.sqrt(1000 * 50 / 10000)
    assert gsd == 0.5 * f and (w, h) == (int(1000 / f), int(50 / f))
    assert host.ortho_clamp_megapixels(0.0, 0.5, 1000, 50) == (0.5, 1000, 50)
    assert host.ortho_clamp_megapixels(float("nan"), 0.5, 1000, 50) == (0.5, 1000, 50)
    assert host.ortho_clamp_megapixels(1e-7, 0.5, 1000, 50) == (0.5, 1000, 50)      # max_output_pixels == 0
    assert host.ortho_clamp_megapixels(1e-6, 0.5, 1000, 1)[1:] == (31, 1)           # max(1, .)
    assert host.ortho_clamp_megapixels(0.05, 0.5, 1000, 50) == (0.5, 1000, 50)      # at the cap


def test_degenerate_bounds_give_100_pixels():
    """A surface of one point has zero extent: the preview (size < 1 as a double) and the DSM (size <= 0 after
    truncation) both fall back to 100 x 100."""
    pos, ori, model, thumbs = three_cameras()
    g = make_graph(pos, ori, model, thumbs)
    s = cloud_surface([(5, 5, 0)])
    t = host.orthomosaic_thumbnail(g, [s])
    d = host.dsm_plan(g, [s])
    assert (t["width"], t["height"]) == (100, 100) and (d["width"], d["height"]) == (100, 100)
    g.close()


def test_cpu_preview_samples_the_distorted_projection():
    """With radial and tangential distortion: every pixel the CPU route colours from a camera shows the thumbnail cell
    that the reference's image_from_3d (restated in numpy here, distort_keypoints.hpp:26-86) gives for the pixel's
    3-D point in that camera (the thumbnails encode their own column and row)."""
    pos, ori = jittered_cameras(4, 3, seed=11)
    model = [400, 205, 148, 0.05, -0.01, 0.002, 0.003, -0.002, 400, 300]
    rows, cols = 120, 160
    cell = np.zeros((rows, cols, 3), np.uint8)
    cell[..., 0] = np.arange(cols)[None, :]
    cell[..., 1] = np.arange(rows)[:, None]
    g = make_graph(pos, ori, model, [cell] * len(pos))
    s = perturbed_mesh(pos, seed=11)
    out = host.orthomosaic_thumbnail(g, [s], want_z=True)
    lit = np.nonzero(out["rgba"][..., 3] == 255)
    assert len(lit[0]) > 1000
    index = {nid & 0xFFFFFFFF: i for i, nid in enumerate(g.node_ids)}
    got = out["rgba"][lit][:, :2].astype(np.int64)
    xs, ys = pixel_centres(out)
    exp = np.zeros_like(got)
    for k, (r, c) in enumerate(zip(*lit)):
        i = index[int(out["ids"][r, c])]
        px = project(np.array([xs[r, c], ys[r, c], out["z"][r, c]]), pos[i], ori[i], model)
        exp[k] = (px * (rows / model[9])).astype(np.int64)
    assert np.abs(got - exp).max() <= 1 and (got == exp).all(axis=1).mean() > 0.999
    g.close()


def test_set_thumbnail_refuses_sizes_the_device_cannot_sample():
    pos, ori, model, thumbs = three_cameras()
    g = make_graph(pos, ori, model)
    with pytest.raises(ValueError):
        g.set_thumbnail(0, np.zeros((1, 65536, 3), np.uint8))
    with pytest.raises(ValueError):
        g.set_thumbnail(0, np.zeros((0, 5, 3), np.uint8))
    g.set_thumbnail(0, np.zeros((1, 65535, 3), np.uint8))
    g.close()

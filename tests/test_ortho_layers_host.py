"""The layered full-resolution orthomosaic on the host (csrc/host/ortho_layers.cpp, csrc/ortho_layers.hpp): the
reference's known answers of PatchSampler and computeBlendWeight (test/test_ortho.cpp:700-780, test/test_blending.cpp:
11-38), departure L1's colour conversion against published CIE values, and the CPU route against a numpy restatement of
the per-pixel camera choice and the correspondence sampling rules."""
import numpy as np
import pytest

from layers_fixtures import DISTORTED, expected_layers, knn_agrees, four_camera_scene, plan_with_gsd
from layers_oracle_fixtures import blend_weight_f32, correspondences, ld, mean_bound
from ortho_fixtures import DOWN, make_graph, project
from opencalibration_amd import host

REF_MODEL = [500, 50, 50, 0, 0, 0, 0, 0, 100, 100]  # test_ortho.cpp:700-780


def ref_camera():
    """the camera of test_ortho.cpp:700-780: (0, 0, 10), AngleAxis(pi, X), f 500, 100 x 100"""
    g = make_graph([(0, 0, 10)], [DOWN], REF_MODEL)
    cam = host.ortho_layers_cameras(g, [])["cams"][0]
    g.close()
    return cam


def test_patch_sampler_jacobian():                                      # test_ortho.cpp:700-724
    _, _, J = host.ortho_patch_sample(ref_camera(), np.zeros((100, 100, 3), np.uint8), 0.01, [0, 0, 0])
    assert abs(abs(J[0, 0]) - 50) < 1e-6 and abs(abs(J[1, 1]) - 50) < 1e-6
    assert abs(J[0, 1]) < 1e-6 and abs(J[1, 0]) < 1e-6


def test_patch_sampler_single_pixel():                                  # test_ortho.cpp:727-752
    img = np.broadcast_to(np.array([100, 150, 200], np.uint8), (100, 100, 3))
    bgr, _, _ = host.ortho_patch_sample(ref_camera(), img, 0.01, [0, 0, 0])
    assert bgr is not None and bgr.tolist() == [100, 150, 200]


def test_patch_sampler_averaging():                                     # test_ortho.cpp:755-780
    yy, xx = np.mgrid[:100, :100]
    img = np.zeros((100, 100, 3), np.uint8)
    img[(xx - 50) ** 2 + (yy - 50) ** 2 <= 100] = 255  # cv::circle(.., 10, white, filled)
    bgr, _, _ = host.ortho_patch_sample(ref_camera(), img, 0.5, [0, 0, 0])
    assert bgr is not None and 50 < bgr[0] < 255


def test_blend_weight_orderings():                                      # test_blending.cpp:11-38
    w = lambda x, y, d: host.ortho_sample_fields(x, y, 100, 100, d)[3]
    assert w(50, 50, 10.0) > 0
    assert w(0, 50, 10.0) < w(50, 50, 10.0)
    assert w(50, 50, 5.0) > w(50, 50, 50.0)


def test_sample_fields_exact_float32():
    """normalizedImageRadius, normalizedImagePosition (ortho.cpp:43-67) and computeBlendWeight (blending.cpp:12-36), in
    numpy with the reference's float / double steps"""
    rng = np.random.default_rng(0)
    f32 = np.float32
    for _ in range(300):
        w, h = int(rng.integers(50, 4000)), int(rng.integers(50, 3000))
        x, y = rng.uniform(-5, w + 5), rng.uniform(-5, h + 5)
        d = f32(rng.uniform(0, 200))
        got = host.ortho_sample_fields(x, y, w, h, d)
        hw, hh = w * 0.5, h * 0.5
        r = np.clip(np.sqrt(((x - hw) / hw) ** 2 + ((y - hh) / hh) ** 2) * 0.7071067811865475, 0, 1)
        nx = np.clip(f32((x - hw) / hw), f32(-1), f32(1))
        ny = np.clip(f32((y - hh) / hh), f32(-1), f32(1))
        wt = blend_weight_f32(f32(x), f32(y), w, h, d)
        assert got[0] == f32(r) and got[1] == nx and got[2] == ny and got[3] == wt


def test_view_angle_restatement():
    for c in np.linspace(-1, 1, 2001):
        assert abs(host.ortho_sample_fields(1, 1, 10, 10, 1.0, c)[4] - np.float32(np.arccos(c))) <= 2e-7 * (1 + np.arccos(c))


def test_l1_float_path_white_black_and_primaries():
    lab = host.lab_convert([[255, 255, 255], [0, 0, 0], [0, 0, 255], [0, 255, 0], [255, 0, 0]], "bgr2labf")
    assert np.allclose(lab[0], [100, 0, 0], atol=1e-4) and np.array_equal(lab[1], [0, 0, 0])
    textbook = [[53.2408, 80.0925, 67.2032], [87.7347, -86.1827, 83.1793], [32.2970, 79.1875, -107.8602]]  # sRGB R, G, B
    assert np.abs(lab[2:] - textbook).max() < 0.05


def test_l1_greys_are_neutral_on_the_8bit_path():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    lab8 = host.lab_convert(grey, "bgr2lab8")
    assert np.all(lab8[:, 1:] == 128)
    assert lab8[0, 0] == 0 and lab8[255, 0] == 255 and np.all(np.diff(lab8[:, 0].astype(int)) >= 0)
    back = host.lab_convert(lab8, "lab82bgr").astype(int)
    assert np.all(back == back[:, :1]) and np.abs(back[:, 0] - np.arange(256)).max() <= 2  # L's 8-bit grid: 100 / 255


def test_l1_8bit_round_trip_bound():
    """BGR -> 8-bit Lab -> BGR over 10^5 seeded colours: within 24 codes per channel (Lab's 8-bit grid is coarse in the
    dark and saturated corners); 95 % come back within 4"""
    bgr = np.random.default_rng(1).integers(0, 256, (100000, 3), dtype=np.uint8)
    back = host.lab_convert(host.lab_convert(bgr, "bgr2lab8"), "lab82bgr")
    err = np.abs(back.astype(int) - bgr.astype(int)).max(axis=1)
    assert err.max() <= 24 and (err <= 4).mean() > 0.95


def route(plan, g, s, imgs, cfg, **kw):
    return host.ortho_layers(plan, g, [s], imgs, config=cfg, debug_knn=True, **kw)


@pytest.fixture(scope="module")
def scene():
    g, s, imgs = four_camera_scene()
    plan = dict(width=210, height=150, gsd=0.05, min_x=-2.0, max_x=8.5, min_y=-1.0, max_y=6.5, mean_camera_z=10.0)
    yield g, s, imgs, plan
    g.close()


def test_cpu_route_camera_choice_against_numpy(scene):
    g, s, imgs, plan = scene
    out = route(plan, g, s, imgs, dict(num_layers=3, tile_size=64, correspondence_subsample=9))
    dsm = host.dsm_render(plan, [s])
    cams = host.ortho_layers_cameras(g, [s])
    knn, _ = expected_layers(plan, cams["cams"], g.orientations(), cams["cams"][:, :3], [DISTORTED] * 4, dsm * np.nan, 3)
    assert knn_agrees(out["knn"], knn, plan, cams["cams"])
    _, layers = expected_layers(plan, cams["cams"], g.orientations(), cams["cams"][:, :3], [DISTORTED] * 4, dsm, 3,
                                order_in=out["knn"])
    idx = {int(n): i for i, n in enumerate(cams["node_ids"])}
    got = np.vectorize(lambda v: idx.get(int(v), -1))(out["camera_id"])
    assert np.array_equal(got, layers)
    valid = out["bgra"][..., 3] == 255
    assert np.array_equal(valid, layers >= 0) and valid[2].any()
    assert not (valid[1:] & ~valid[:-1]).any()
    assert np.all(out["bgra"][~valid] == 0) and np.all(out["camera_id"][~valid] == 0) and np.all(out["weight"][~valid] == 0)
    assert np.all(out["weight"][valid] > 0)


def test_single_pixel_and_ellipse_paths(scene):
    """small gsd: every sample is the source pixel under the projection (truncated); large gsd: the ellipse averages
    (many samples differ from the centre pixel of noise images)"""
    g, s, imgs, plan = scene
    cams = host.ortho_layers_cameras(g, [s])
    ori = g.orientations()
    for gsd, single in ((0.02, True), (0.3, False)):
        p = plan_with_gsd(plan, gsd)
        out = route(p, g, s, imgs, dict(num_layers=1, correspondence_subsample=0))
        dsm = host.dsm_render(p, [s])
        idx = {int(n): i for i, n in enumerate(cams["node_ids"])}
        rows, cols = np.nonzero(out["bgra"][0, ..., 3] == 255)
        pick = np.random.default_rng(0).choice(len(rows), min(300, len(rows)), replace=False)
        same = 0
        for r, c in zip(rows[pick], cols[pick]):
            i = idx[int(out["camera_id"][0, r, c])]
            pt = [c * p["gsd"] + p["min_x"], p["max_y"] - r * p["gsd"], float(dsm[r, c])]
            px = project(pt, cams["cams"][i, :3], ori[i], DISTORTED)
            same += np.array_equal(out["bgra"][0, r, c, :3], imgs[i][int(px[1]), int(px[0])])
        if single:
            assert same == len(pick)
        else:
            assert same < len(pick) // 2


def numpy_sampled(cam0, valid, tile, sub):
    """the boundary and subsample rules of ortho.cpp:1324-1353 on layer-0 camera ids, tile-local"""
    rows, cols = cam0.shape
    out = np.zeros((rows, cols), bool)
    for r0 in range(0, rows, tile):
        for c0 in range(0, cols, tile):
            ids, ok = cam0[r0:r0 + tile, c0:c0 + tile], valid[r0:r0 + tile, c0:c0 + tile]
            th, tw = ids.shape
            b = np.zeros((th, tw), bool)
            b[:, 1:] |= ok[:, :-1] & (ids[:, :-1] != ids[:, 1:])
            b[:, :-1] |= ok[:, 1:] & (ids[:, 1:] != ids[:, :-1])
            b[1:, :] |= ok[:-1, :] & (ids[:-1, :] != ids[1:, :])
            b[:-1, :] |= ok[1:, :] & (ids[1:, :] != ids[:-1, :])
            lr, lc = np.mgrid[:th, :tw]
            samp = np.where(b, (lr + lc) % sub == 0, (lr % sub == 0) & (lc % sub == 0))
            out[r0:r0 + th, c0:c0 + tw] = samp & ok
    return out


@pytest.mark.parametrize("tile", [64, 40])
def test_correspondences_cpu_route(scene, tile):
    g, s, imgs, plan = scene
    sub = 7
    out = route(plan, g, s, imgs, dict(num_layers=3, tile_size=tile, correspondence_subsample=sub))
    cor = out["correspondences"]
    valid = out["bgra"][..., 3] == 255
    nvalid = valid.sum(0)
    expect = numpy_sampled(out["camera_id"][0], valid[0], tile, sub) & (nvalid >= 2)
    got = np.zeros_like(expect)
    got[cor["row"], cor["col"]] = True
    assert np.array_equal(got, expect) and expect.sum() > 10
    # one record per pair of valid layers, the pair's ids at the pixel
    assert len(cor) == int((nvalid * (nvalid - 1) // 2)[expect].sum())
    assert np.array_equal(cor["camera_id_a"], out["camera_id"][cor["layer_a"], cor["row"], cor["col"]])
    assert np.array_equal(cor["camera_id_b"], out["camera_id"][cor["layer_b"], cor["row"], cor["col"]])
    assert np.all(cor["layer_a"] < cor["layer_b"]) and np.all(cor["camera_id_a"] != cor["camera_id_b"])
    # canonical order: tiles row-major, local raster order, then (a, b)
    key = np.stack([cor["row"] // tile, cor["col"] // tile, cor["row"] % tile, cor["col"] % tile, cor["layer_a"],
                    cor["layer_b"]], 1)
    assert np.all(np.diff(np.lexsort(key.T[::-1])) == 1)
    # each mean against the long-double mean of the window's reference Lab, within float summation's forward bound
    exp = correspondences(out["bgra"], out["camera_id"], tile, 2, sub)
    assert [(e["row"], e["col"]) for e in exp] == list(zip(cor["row"].tolist(), cor["col"].tolist()))
    for side in "ab":
        mean = np.array([e["mean_" + side] for e in exp])
        bound = np.array([mean_bound(e["count"], e["abs_" + side]) for e in exp])
        assert np.all(np.abs(ld(cor["lab_" + side]) - mean) <= bound)


def test_tile_size_moves_the_boundary_set(scene):
    """the boundary test only looks inside the tile: at tile edges a different tile size changes which pixels are
    boundary pixels, exactly as the tile-local rule predicts"""
    g, s, imgs, plan = scene
    res = {}
    for tile in (64, 50):
        out = route(plan, g, s, imgs, dict(num_layers=2, tile_size=tile, correspondence_subsample=3))
        cor = out["correspondences"]
        got = np.zeros((plan["height"], plan["width"]), bool)
        got[cor["row"], cor["col"]] = True
        valid = out["bgra"][..., 3] == 255
        res[tile] = got
        assert np.array_equal(got, numpy_sampled(out["camera_id"][0], valid[0], tile, 3) & valid[1])
    assert not np.array_equal(res[64], res[50])


def test_bands_equal_one_call_and_bad_arguments(scene):
    g, s, imgs, plan = scene
    cfg = dict(tile_size=32, correspondence_subsample=5)
    whole = route(plan, g, s, imgs, cfg)
    bands = list(host.ortho_layers_bands(plan, g, [s], imgs, tile_rows=2, config=cfg))
    assert len(bands) == -(-plan["height"] // 64)
    assert np.array_equal(np.concatenate([b["bgra"] for b in bands], 1), whole["bgra"])
    assert np.concatenate([b["correspondences"] for b in bands]).tobytes() == whole["correspondences"].tobytes()
    with pytest.raises(ValueError):
        host.ortho_layers(plan, g, [s], imgs, row0=5, config=cfg)
    with pytest.raises(Exception):
        host.ortho_layers(plan, g, [s], [im[:-1] for im in imgs], config=cfg)

"""The scenes of the layered orthomosaic's reference tests (test_ortho_layers_oracle.py on the CPU route,
layers_oracle_gpu_child.py on the device) and the one comparison both routes go through: a route's planes and records
against layers_oracle_fixtures' long-double reference, fed the route's own kNN lists and heights."""
import numpy as np

import layers_oracle_fixtures as ref
from layers_fixtures import noise_images, plan_with_gsd
from ortho_fixtures import DOWN, cloud_surface, make_graph, qmul, quat
from opencalibration_amd import host

# f ppx ppy k1 k2 k3 p1 p2 cols rows: every coefficient non-zero
FULL_MODEL = [100, 80, 60, -0.05, 0.01, 0.002, 0.001, -0.0005, 160, 120]
BOUNDS = dict(min_x=-2.0, max_x=8.5, min_y=-1.0, max_y=6.5, mean_camera_z=10.0, width=0, height=0, gsd=0.0)
FOUR = [(0, 0, 10), (6, 0.3, 10), (0.2, 5, 10.5), (6.5, 5.2, 9.5)]
CLOUD = [(-4, -4, 0), (10, -4, 0), (10, 9, 0), (-4, 9, 0), (3, 2.5, 0.5)]
AMBIGUOUS_SHARE = 0.002


def oblique(yaw_deg, tilt_deg):
    """a downward camera tilted about the world's x axis, then turned about the vertical"""
    return qmul(quat((0, 0, 1), np.radians(yaw_deg)), qmul(quat((1, 0, 0), np.radians(tilt_deg)), DOWN))


class Scene:
    def __init__(self, pos, ori, plan, cfg, seed, second_surface=False):
        self.pos, self.ori, self.plan, self.cfg = pos, ori, plan, cfg
        self.graph = make_graph(pos, ori, FULL_MODEL)
        s = host.rebuild_mesh(np.array(pos, np.float64), previous=cloud_surface(CLOUD))
        self.surfaces = [s]
        if second_surface:
            self.surfaces.append(host.rebuild_mesh(np.array(pos[:3], np.float64),
                                                   previous=cloud_surface([(-6, -6, 1), (12, -6, 1), (12, 11, 1), (-6, 11, 1)])))
        self.images = noise_images(len(pos), FULL_MODEL[9], FULL_MODEL[8], seed)

    def close(self):
        self.graph.close()


def tilted_four(seed):
    rng = np.random.default_rng(seed)
    return [qmul(quat(rng.normal(size=3), 0.04), DOWN) for _ in FOUR]


def scene_a():
    """four_camera_scene with k3 = 0.002, 95 x 68 at gsd 0.11: partial 64-pixel tiles, ellipses of radius 2 that at two
    samples hold no pixel centre.  (With this model a stays above 1.006 at gsd 0.11: the single-pixel path and its
    meeting with the ellipse path are scene D's.)"""
    return Scene(FOUR, tilted_four(0), plan_with_gsd(BOUNDS, 0.11),
                 dict(num_layers=3, tile_size=64, correspondence_subsample=7, correspondence_kernel_radius=2), 0)


def scene_b():
    """the same at gsd 0.3, 35 x 25: every sample an ellipse of radius 3 - 4, windows clipped at the image borders"""
    return Scene(FOUR, tilted_four(0), plan_with_gsd(BOUNDS, 0.3),
                 dict(num_layers=3, tile_size=64, correspondence_subsample=3, correspondence_kernel_radius=2), 0)


def scene_c():
    """the same at gsd 2.5, 4 x 3: the 16-pixel radius cap"""
    return Scene(FOUR, tilted_four(0), plan_with_gsd(BOUNDS, 2.5),
                 dict(num_layers=3, tile_size=64, correspondence_subsample=1, correspondence_kernel_radius=2), 0)


def scene_d():
    """four oblique cameras (yaw -40 .. 40 degrees, tilt 20 - 30), 77 x 54 at gsd 0.11: J far from isotropic, M far from
    diagonal; of 10 358 samples 919 take the single-pixel path (a < 1), 2 810 (27 %) have a > 1 > b, the rest b > 1"""
    ori = [oblique(-40, 20), oblique(-13, 30), oblique(13, 23), oblique(40, 27)]
    return Scene(FOUR, ori, plan_with_gsd(dict(BOUNDS, min_x=0.0, min_y=0.0, max_y=6.0), 0.11),
                 dict(num_layers=3, tile_size=32, correspondence_subsample=5, correspondence_kernel_radius=2), 5)


def scene_e():
    """44 x 44 at gsd 0.68 over a corner of the mesh: 416 pixels off it (NaN heights, every layer invalid), a fifth
    camera that looks up (ray z <= 0: skipped 1 520 times), a second surface, ellipses of radius 7 - 8"""
    pos = FOUR + [(3, 2.5, 10.2)]
    ori = tilted_four(2) + [quat((1, 2, 0), 0.1)]
    plan = plan_with_gsd(dict(BOUNDS, min_x=-23.0, max_x=7.0, min_y=-22.0, max_y=8.0), 0.68)
    return Scene(pos, ori, plan, dict(num_layers=3, tile_size=32, correspondence_subsample=4,
                                      correspondence_kernel_radius=2), 2, second_surface=True)


def expect_a(s):
    assert s["ellipse"] > 10000 and s["outside"] > 0 and s["empty"] > 0


def expect_b(s):
    assert s["single"] == 0 and s["clipped"] > 0 and 3 <= s["max_radius"] <= 4


def expect_c(s):
    assert s["capped"] > 0 and s["max_radius"] == 16


def expect_d(s):
    assert s["a_over_1_over_b"] > 0.25 * (s["single"] + s["ellipse"]) and s["single"] > 500


def expect_e(s):
    assert s["nan"] > 0 and s["behind"] > 0 and s["ellipse"] > 0


SCENES = {"A": (scene_a, expect_a), "B": (scene_b, expect_b), "C": (scene_c, expect_c), "D": (scene_d, expect_d),
          "E": (scene_e, expect_e)}


def check_route(scene, out, dsm, expect):
    """out: a route's result with debug_knn=True, dsm: the float heights it rendered.  Asserts bgra, camera ids and
    weights on every unambiguous pixel and layer, every record's fields and means, the ambiguity cap and that the scene
    took the branches it exists for; returns the counts."""
    cams = host.ortho_layers_cameras(scene.graph, scene.surfaces)
    assert len(cams["node_ids"]) == len(scene.pos)
    C = ref.Cameras(scene.pos, scene.ori, FULL_MODEL)
    L, cfg = scene.cfg["num_layers"], scene.cfg
    r = ref.render(scene.plan, C, [ref.Image(im) for im in scene.images], cams["node_ids"], out["knn"], dsm, L)
    amb = r["ambiguous"]
    stats = dict(r["stats"], pixels=int(amb.size), ambiguous=int(amb.sum()), records=len(out["correspondences"]))
    print("layers oracle:", stats)
    assert stats["ambiguous"] <= int(AMBIGUOUS_SHARE * amb.size), stats
    expect(stats)
    clear = ~amb
    assert np.array_equal(out["bgra"][:, clear], r["bgra"][:, clear])
    assert np.array_equal(out["camera_id"][:, clear], r["camera_id"][:, clear])
    assert np.array_equal(out["weight"][:, clear].view(np.uint32), r["weight"][:, clear].view(np.uint32))
    # the records: which, in which order, and every field
    cor = out["correspondences"]
    exp = ref.correspondences(out["bgra"], out["camera_id"], cfg["tile_size"], cfg["correspondence_kernel_radius"],
                              cfg["correspondence_subsample"])
    assert len(cor) == len(exp) and len(exp) > 0
    for key in ("row", "col", "layer_a", "layer_b"):
        assert np.array_equal(cor[key], np.array([e[key] for e in exp])), key
    for side in "ab":
        at = (cor["layer_" + side].astype(np.int64), cor["row"], cor["col"])
        ok = clear[cor["row"], cor["col"]]
        assert ok.any()
        assert np.array_equal(cor["camera_id_" + side][ok], r["camera_id"][at][ok])
        assert np.array_equal(cor["model_id_" + side][ok], cams["model_ids"][r["camera"][at]][ok])
        for k, name in enumerate(("normalized_radius_", "normalized_x_", "normalized_y_", "view_angle_")):
            got, want = cor[name + side][ok], r["fields"][at][ok][:, k]
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name + side
        mean = np.array([e["mean_" + side] for e in exp])
        bound = np.array([ref.mean_bound(e["count"], e["abs_" + side]) for e in exp])
        err = np.abs(ref.ld(cor["lab_" + side]) - mean)
        stats["lab_worst"] = max(stats.get("lab_worst", 0.0), float((err / np.maximum(bound, ref.LD("1e-300"))).max()))
        assert np.all(err <= bound), (side, float((err - bound).max()))
    return stats

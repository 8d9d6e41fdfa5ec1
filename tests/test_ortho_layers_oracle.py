"""The per-pixel rules of the layered orthomosaic (csrc/ortho_layers.hpp) on the CPU route against a long-double numpy
reference written from the rules (layers_oracle_fixtures.py): the colour conversions code by code, the projection and
its Jacobian point by point, the ellipse sampler on noise images, and whole scenes (layers_oracle_scenes.py) pixel by
pixel, layer by layer and record by record.  The device route compiles the same header; it meets the same reference in
test_gpu_ortho_layers_oracle.py."""
import numpy as np
import pytest

import layers_oracle_fixtures as ref
from layers_oracle_scenes import FULL_MODEL, SCENES, check_route, oblique
from layers_fixtures import noise_images
from ortho_fixtures import DOWN, make_graph
from opencalibration_amd import host

LD = ref.LD


@pytest.fixture(scope="module")
def colours():
    """all 256 greys, the lattice of every channel in steps of 5, the 8 cube corners and 10^6 seeded colours"""
    grey = np.repeat(np.arange(256)[:, None], 3, 1)
    step = np.arange(0, 256, 5)
    lattice = np.stack(np.meshgrid(step, step, step, indexing="ij"), -1).reshape(-1, 3)
    corners = np.array([[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)])
    rand = np.random.default_rng(7).integers(0, 256, (1000000, 3))
    return np.concatenate([grey, lattice, corners, rand]).astype(np.uint8)


def test_8bit_conversions_code_by_code(colours):
    """BGR -> 8-bit Lab and 8-bit Lab -> BGR over the colour set (read as Lab codes on the way back): equal wherever the
    unrounded value is at least 1e-9 from a rounding tie; at most 10 colours nearer than that (none today: over all 2^24
    the nearest is 2.5e-9 of a code forward and 1.8e-8 back)"""
    for mode, fn in (("bgr2lab8", ref.bgr2lab8), ("lab82bgr", ref.lab82bgr)):
        want, margin = fn(colours)
        clear = margin >= ref.EDGE
        print(mode, "ambiguous", int((~clear).sum()), "smallest margin", float(margin.min()))
        assert (~clear).sum() <= 10
        assert np.array_equal(host.lab_convert(colours, mode)[clear], want[clear]), mode


def float_conversion_agrees(bgr, channels):
    want, tie = ref.bgr2labf(bgr)
    got = host.lab_convert(bgr, "bgr2labf")
    want, tie, got = want[:, channels], tie[:, channels], got[:, channels]
    same = got == want
    one_ulp = (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))
    print("float Lab: differ", int((~same).sum()), "on a tie", int(tie.sum()), "largest", np.abs(got - want).max())
    return np.all(same | (tie & one_ulp))


def test_float_conversion_is_the_rounded_reference(colours):
    """BGR -> float Lab: the float32 of the long-double value, or one ulp off where that value lies within 1e-9
    (relative) of a float32 tie.  Every colour's L, and a and b of every colour that is not a grey (those: the test below)."""
    grey = (colours[:, 0] == colours[:, 1]) & (colours[:, 1] == colours[:, 2])
    assert float_conversion_agrees(colours, [0]) and float_conversion_agrees(colours[~grey], [1, 2])


def test_float_conversion_of_greys():
    """The same for a and b of the 256 greys, whose exact value is 0 (each matrix row sums to its white): 0 to the bit.
    The header takes X / Xn, Y and Z / Zn as G plus multiples of R - G and B - G for this; as plain row sums its doubles
    left a and b of 154 of these 512 values at up to 1.1e-13, which is the float32 of nothing near 0."""
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    assert float_conversion_agrees(grey, [1, 2])
    assert np.all(host.lab_convert(grey, "bgr2labf")[:, 1:] == 0)


# ---- projection, Jacobian and sampler, point by point ------------------------------------------------------------------
CAMERAS = {
    "nadir": (DOWN, [100, 80, 60, 0, 0, 0, 0, 0, 160, 120]),
    "oblique": (oblique(35, 25), [100, 80, 60, 0, 0, 0, 0, 0, 160, 120]),
    "distorted": (oblique(35, 25), FULL_MODEL),
}
POSITION = (1.0, -2.0, 10.0)


def camera(name):
    ori, model = CAMERAS[name]
    g = make_graph([POSITION], [ori], model)
    cam = host.ortho_layers_cameras(g, [])["cams"][0]
    g.close()
    return cam, ref.Cameras([POSITION], [ori], model)


def ground_points(C, n, seed):
    """n seeded points around where the camera's axis meets the ground: most inside the image, some outside"""
    axis = np.asarray(C.R_inv[0][2], np.float64)
    hit = np.array(POSITION) - axis * (POSITION[2] / axis[2])
    rng = np.random.default_rng(seed)
    return hit + rng.uniform([-9, -7, -0.5], [9, 7, 0.5], (n, 3))


def test_reference_jacobian_against_central_differences():
    for name in CAMERAS:
        _, C = camera(name)
        p = ground_points(C, 50, 1)
        ci, h = np.zeros(len(p), int), LD("1e-5")
        _, _, J = ref.project(C, ci, *p.T)
        for k in range(2):
            d = np.zeros(3, LD)
            d[k] = h
            hi = ref.project(C, ci, *(ref.ld(p) + d).T, jacobian=False)[1]
            lo = ref.project(C, ci, *(ref.ld(p) - d).T, jacobian=False)[1]
            assert np.abs((hi - lo) / (2 * h) - J[:, :, k]).max() < 1e-6 * np.abs(J).max()


@pytest.mark.parametrize("name", list(CAMERAS))
def test_patch_sample_point_by_point(name):
    """pixel and J to 1e-12 of their size at 500 seeded points, the colour on a noise image (gsd 0.04 - 0.5: both paths)
    wherever the reference is not ambiguous; nothing where the pixel falls outside"""
    cam, C = camera(name)
    img = noise_images(1, 120, 160, 11)[0]
    pts = ground_points(C, 500, 3)
    gsd = np.random.default_rng(4).uniform(0.04, 0.5, len(pts))
    rz, pixel, J = ref.project(C, np.zeros(len(pts), int), *pts.T)
    inside = (rz > 0) & (pixel[:, 0] >= 0) & (pixel[:, 0] < 160) & (pixel[:, 1] >= 0) & (pixel[:, 1] < 120)
    edge = ref.near(pixel[:, 0], 0) | ref.near(pixel[:, 0], 160) | ref.near(pixel[:, 1], 0) | ref.near(pixel[:, 1], 120)
    want = np.zeros((len(pts), 3), np.uint8)
    amb = np.zeros(len(pts), bool)
    want[inside], amb[inside], info = ref.sample(ref.Image(img), pixel[inside], J[inside], gsd[inside])
    assert info["single"].sum() > 30 and (~info["single"]).sum() > 30 and (~inside).sum() > 10
    checked = 0
    for k in range(len(pts)):
        bgr, px, Jk = host.ortho_patch_sample(cam, img, gsd[k], pts[k])
        assert np.abs(px - pixel[k]).max() <= 1e-12 * max(1, np.abs(pixel[k]).max())
        assert np.abs(Jk - J[k]).max() <= 1e-12 * np.abs(J[k]).max()
        if edge[k] or amb[k]:
            continue
        assert (bgr is not None) == inside[k]
        if inside[k]:
            assert bgr.tolist() == want[k].tolist(), (k, gsd[k])
            checked += 1
    assert checked > 300


def test_ray_z_clamp():
    """0 < ray z < 1e-3: the ray is divided by 1e-3 and that z is a constant to the Jacobian, the sample is taken; ray z
    <= 0: the same pixel rule, no sample"""
    cam, C = camera("nadir")
    img = noise_images(1, 120, 160, 12)[0]
    for z, taken in ((POSITION[2] - 5e-4, True), (POSITION[2] + 0.5, False)):
        p = np.array([POSITION[0] + 1.234e-5, POSITION[1] - 2.345e-5, z])
        rz, pixel, J = ref.project(C, [0], *p[:, None])
        assert (0 < rz[0] < 1e-3) == taken and (rz[0] <= 0) != taken
        assert np.abs(J).max() > 9e4  # f / 1e-3
        bgr, px, Jk = host.ortho_patch_sample(cam, img, 1e-6, p)
        assert np.abs(px - pixel[0]).max() <= 1e-12 * np.abs(pixel[0]).max()
        assert np.abs(Jk - J[0]).max() <= 1e-12 * np.abs(J[0]).max()
        assert (bgr is not None) == taken
        if taken:
            want, amb, _ = ref.sample(ref.Image(img), pixel, J, 1e-6)
            assert not amb[0] and bgr.tolist() == want[0].tolist()


# ---- whole scenes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_cpu_route_against_reference(name):
    """Scenes A - E (layers_oracle_scenes.py) on the CPU route, the reference fed the route's kNN lists and
    host.dsm_render's heights.  Ambiguous pixels on this route: A 0 of 6 460, B 0 of 875, C 0 of 12, D 0 of 4 158, E 0 of
    1 936; the worst Lab mean sits at 0.34 of its summation bound."""
    make, expect = SCENES[name]
    scene = make()
    out = host.ortho_layers(scene.plan, scene.graph, scene.surfaces, scene.images, config=scene.cfg, debug_knn=True)
    dsm = host.dsm_render(scene.plan, scene.surfaces)
    check_route(scene, out, dsm, expect)
    scene.close()

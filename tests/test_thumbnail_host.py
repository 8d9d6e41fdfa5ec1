"""The load stage's thumbnail on the CPU route (csrc/host/thumbnail.cpp over csrc/thumbnail.hpp): bit for bit against the
numpy restatement of thumbnail_fixtures.py on the general and the integer path, the size rule, constant images, the
refusals, and the graph calls - the default load leaves nodes without thumbnails, make_thumbnails feeds the preview."""
import inspect

import numpy as np
import pytest

from ortho_fixtures import DOWN, cloud_surface, make_graph
from thumbnail_fixtures import CPU_SHAPES, SHAPES, cpu_route, images, size_restated, thumbnail_restated
from opencalibration_amd import capi, host


@pytest.mark.parametrize("name", CPU_SHAPES)
def test_cpu_route_equals_restatement(name):
    w, h, batch = SHAPES[name]
    got, src = cpu_route(name), images(name)
    assert got.shape == (batch,) + host.thumbnail_size(w, h) + (3,)
    for i in range(batch):
        assert np.array_equal(got[i], thumbnail_restated(src[i])), i
    assert len(np.unique(got)) > 8  # the images are no constants


@pytest.mark.parametrize("width, height, rows, cols", [(4000, 3000, 43, 58), (173, 131, 44, 57), (4000, 2250, 38, 67),
                                                       (180, 125, 42, 60), (250, 90, 30, 83)])
def test_sizes(width, height, rows, cols):
    assert host.thumbnail_size(width, height) == (rows, cols)
    assert size_restated(width, height)[:2] == (rows, cols)


def test_integer_path_pixel_counts():
    """1 / scale is an integer to within DBL_EPSILON exactly for the shapes named so (4000 x 2250: n = 60)"""
    eps = np.finfo(np.float64).eps
    for name, (w, h, _) in list(SHAPES.items()) + [("integer_4000x2250", (4000, 2250, 1))]:
        inv = size_restated(w, h)[2]
        assert (abs(inv - np.rint(inv)) < eps) == name.startswith("integer"), name
    assert np.rint(size_restated(4000, 2250)[2]) == 60


def test_constant_images():
    """A constant image of colour c gives the constant thumbnail lab82bgr(bgr2lab8(c)), on both paths"""
    rng = np.random.default_rng(5)
    colours = np.concatenate([np.array([(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255)], np.uint8),
                              rng.integers(0, 256, (64, 3), dtype=np.uint8)])
    want = host.lab_convert(host.lab_convert(colours, "bgr2lab8"), "lab82bgr")[:, ::-1]
    for w, h in ((64, 50), (125, 80)):  # general (3 200 pixels), integer (n = 2, 62.5 columns round to 62: one unused)
        batch = np.broadcast_to(colours[:, None, None, :], (len(colours), h, w, 3))
        got = host.image_thumbnails(batch)
        assert np.array_equal(got, np.broadcast_to(want[:, None, None, :], got.shape)), (w, h)


def test_refusals():
    with pytest.raises(ValueError, match="2500"):
        host.thumbnail_size(40, 40)
    with pytest.raises(ValueError, match="2500"):
        host.image_thumbnails(np.zeros((1, 40, 40, 3), np.uint8))
    with pytest.raises(ValueError, match="rounds to 0"):
        host.thumbnail_size(60000, 1)
    L = host.load()
    out = np.zeros((50, 50, 3), np.uint8)
    assert L.och_image_thumbnails(None, None, 1, 100, 100, 0, out.ctypes.data) == -1
    assert b"NULL" in L.och_thumbnail_last_error()
    img = np.zeros((100, 100, 3), np.uint8)
    assert L.och_image_thumbnails(None, img.ctypes.data, 1, 100, 100, 1, out.ctypes.data) == -1  # device images, no context
    g = host.Graph()
    with pytest.raises(capi.OchipError, match="no node"):
        g.make_thumbnails(img[None], [12345])
    g.close()


def test_default_load_makes_no_thumbnails_and_make_thumbnails_feeds_the_preview():
    """Nodes added the way the load stage adds them carry no thumbnail, so the preview refuses them; make_thumbnails on
    the CPU route stores image_thumbnails' pixels, and the preview then equals the one set_thumbnail feeds."""
    assert inspect.signature(host.Graph.load_images).parameters["thumbnails"].default is False
    # functional_ortho_scene's geometry (ortho_fixtures.functional_scene) with 180 x 125 views
    pos, ori, model = [(0, 0, 10), (10, 0, 10)], [DOWN, DOWN], [500, 90, 62.5, 0, 0, 0, 0, 0, 180, 125]
    surface = [host.rebuild_mesh(np.array(pos, np.float64),
                                 previous=cloud_surface([(-2, -2, 0), (12, -2, 0), (12, 2, 0), (-2, 2, 0), (5, 0, 0)]))]
    views = images("integer_180x125")[:1].repeat(2, 0).copy()
    views[1] = 255 - views[1]
    g = make_graph(pos, ori, model)
    with pytest.raises(capi.OchipError, match="thumbnail"):
        host.orthomosaic_thumbnail(g, surface)
    g.make_thumbnails(views, g.node_ids)
    got = host.orthomosaic_thumbnail(g, surface)
    g.close()
    g2 = make_graph(pos, ori, model, list(host.image_thumbnails(views)))
    want = host.orthomosaic_thumbnail(g2, surface)
    g2.close()
    assert np.array_equal(got["rgba"], want["rgba"]) and np.array_equal(got["ids"], want["ids"])
    assert (got["rgba"][..., 3] == 255).any() and len(np.unique(got["ids"])) >= 3

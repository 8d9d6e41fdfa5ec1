"""The filtered point cloud file and the textured OBJ in host loops (csrc/xyz_export.hpp run by host/xyz_export.cpp;
DESIGN.md section 4.16) against the yardstick program tests/xyz_export_driver.cpp (std::map counts, the box walk,
`ostream << double`) and Python's '%g'.  Bytes and integers, equal or not; no device."""
import os

import numpy as np
import pytest

import mesh_points_fixtures as M
import xyz_export_fixtures as F
from opencalibration_amd import capi, host

GEOMETRY = (640, 480, -12.5, 83.25, 0.0371, 0.0371)


# ------------------------------------------------------------------------------------------------------------ the numbers
def test_format_g6_equals_ostream_and_percent_g_on_a_million_values():
    v = F.number_family()
    text, length = host.format_g6(v, fallback=False)
    assert (length > 0).all()                                  # every one of these is the integer formatter's
    assert np.array_equal(text, F.number_family_text())
    assert np.array_equal(length, np.char.str_len(text))
    python = np.array([b"%g" % x for x in v.tolist()], dtype="S16")
    assert np.array_equal(text, python)
    assert len(set(length.tolist())) >= 12 and length.max() == 12   # lengths 1 .. 12 all occur


def test_format_g6_edge_values():
    expected = {0.0: b"0", 999999.5: b"1e+06", 999999.49999999994: b"999999", 99999.95: b"99999.9", 0.0001: b"0.0001",
                9.9999949999e-5: b"9.99999e-05", 2.5e-5: b"2.5e-05", 1e6: b"1e+06", 1e15: b"1e+15", 123456.5: b"123456",
                9.2e18: b"9.2e+18", 1e-5: b"1e-05", 100000.0: b"100000", 1234.5675: b"1234.57"}
    text, length = host.format_g6(F.EDGE_VALUES, fallback=False)
    yard = F.driver_format(F.EDGE_VALUES)
    for v, t, l, y in zip(F.EDGE_VALUES, text.tolist(), length.tolist(), yard):
        assert t == y == b"%g" % v and l == len(y), v
        if v in expected and not np.signbit(v):
            assert y == expected[v], v
    assert text[1] == b"-0" and yard[1] == b"-0"               # negative zero keeps its sign


def test_format_g6_declines_what_it_does_not_cover_and_the_fallback_takes_it():
    own, own_len = host.format_g6(F.FALLBACK_VALUES, fallback=False)
    assert (own_len == 0).all() and (own == b"").all()
    text, length = host.format_g6(F.FALLBACK_VALUES, fallback=True)
    yard = F.driver_format(F.FALLBACK_VALUES)
    assert text.tolist() == yard == [b"%g" % v for v in F.FALLBACK_VALUES]
    assert length.tolist() == [len(y) for y in yard] and max(length) == 13
    special, _ = host.format_g6([np.nan, np.inf, -np.inf], fallback=True)
    assert special.tolist() == F.driver_format([np.nan, np.inf, -np.inf])


# ------------------------------------------------------------------------------------------------------ bounds and text
@pytest.mark.parametrize("name", list(F.cloud_cases()))
def test_bounds_and_text_equal_the_yardstick(name):
    case = F.cloud_cases()[name]
    xyz, surfaces = F.flat(case), F.surfaces_of(case)
    n = len(xyz)
    box, kept, text = F.driver_cloud(xyz, "filter")
    _, kept_all, text_all = F.driver_cloud(xyz, None)
    _, kept_box, text_box = F.driver_cloud(xyz, F.CUSTOM_BOX)
    # what the issue states about each cloud, asserted on the yardstick's own result
    assert kept_all == n and text_all.count(b"\n") == n and text.count(b"\n") == kept
    keys = xyz.astype(np.int64)
    if name == "empty":
        assert box == ((0, 0),) * 3 and text == b"" and n == 0
    if name == "one_point":
        assert box == ((12, 12), (-7, -7), (103, 103)) and kept == 1 and text == b"12.25,-7.5,103.062\n"
    if name == "one_cell":
        assert box == ((3, 3),) * 3 and kept == n == 50
    if name == "flat_z":
        assert box[2] == (5, 5) and box[0][0] != box[0][1] and kept == 0 and text == b""
    if name in ("n39", "n40"):
        lo, top, below = keys[:, 0].min(), np.unique(keys[:, 0])[-1], np.unique(keys[:, 0])[-2]
        high = top if name == "n39" else below                 # cutoff 0: the walks do not move; cutoff 1: one cell each end
        assert int(n * 0.025) == (0 if name == "n39" else 1)
        assert box[0] == (high - 2 * (high - lo), high + 2 * (high - lo))
    if name == "straddle_zero":
        assert (np.abs(xyz[-2:]) == 0.9).sum() == 4 and (keys[-2:] == 0).all()   # -0.9 and 0.9 share cell 0
        assert 0 < kept
    if name == "survey":
        assert 0 < kept < n and kept > 0.9 * n
        far = np.abs(xyz).max(1) > 700
        assert far.any() and not any(b"%g,%g,%g\n" % tuple(p) in text for p in xyz[far])
    if name == "far_point":
        assert keys[:, 0].max() == 10 ** 12 and 0 < kept < n and b"1e+12" not in text and b"1e+12,3,-48\n" in text_all
    if name == "two_by_two":
        first, last = xyz[0], xyz[-1]
        assert text_all.startswith(b"%g,%g,%g\n" % tuple(first)) and text_all.endswith(b"%g,%g,%g\n" % tuple(last))
    # the host route
    assert host.cloud_outlier_bounds(surfaces) == box
    assert host.cloud_outlier_bounds(xyz) == box
    assert host.cloud_to_xyz(surfaces, want_kept=True) == (text, kept)
    assert host.cloud_to_xyz(surfaces, bounds=None, want_kept=True) == (text_all, kept_all)
    assert host.cloud_to_xyz(surfaces, bounds=F.CUSTOM_BOX, want_kept=True) == (text_box, kept_box)
    assert host.cloud_to_xyz(xyz, bounds=box) == text
    assert host.cloud_to_xyz(surfaces, bounds=((0, 0),) * 3) == text_all    # the empty box is "no filter", as in the reference


def test_cloud_order_is_surface_cloud_point():
    case = F.cloud_cases()["two_by_two"]
    swapped = [case[1], case[0]]
    a, b = host.cloud_to_xyz(F.surfaces_of(case), bounds=None), host.cloud_to_xyz(F.surfaces_of(swapped), bounds=None)
    assert a != b and sorted(a.split(b"\n")) == sorted(b.split(b"\n"))
    assert b == F.driver_cloud(F.flat(swapped), None)[2]


def test_fallback_numbers_inside_a_cloud():
    xyz = F.survey_cloud(300, 0)
    xyz[100] = [1e-7, 5.0, -48.0]
    xyz[101, 1] = 1e300
    xyz[102, 2] = 5e-324
    _, _, text = F.driver_cloud(xyz, None)
    assert b"1e-07,5,-48\n" in text and b"1e+300" in text and b"4.94066e-324\n" in text
    assert host.cloud_to_xyz(xyz, bounds=None) == text


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 2.0 ** 63, -2.0 ** 63, 1e300])
def test_a_coordinate_without_a_cell_is_refused(bad):
    xyz = F.survey_cloud(200, 0)
    xyz[77, 1] = bad
    with pytest.raises(capi.OchipError, match="not finite or not below 2\\^63"):
        host.cloud_outlier_bounds(xyz)
    with pytest.raises(capi.OchipError, match="not finite or not below 2\\^63"):
        host.cloud_to_xyz([host.Surface().set_clouds([xyz])])
    xyz[77, 1] = np.nextafter(2.0 ** 63, 0)                    # the largest coordinate that has a cell
    assert host.cloud_outlier_bounds(xyz) == F.driver_cloud(xyz, "filter")[0]


def test_save_pointcloud_writes_the_filtered_file(tmp_path):
    surfaces = F.surfaces_of(F.cloud_cases()["two_by_two"])
    box = host.save_pointcloud(tmp_path / "cloud.xyz", surfaces)
    assert box == host.cloud_outlier_bounds(surfaces)
    assert (tmp_path / "cloud.xyz").read_bytes() == host.cloud_to_xyz(surfaces) != b""
    with pytest.raises(capi.OchipError, match="cannot write"):
        host.save_pointcloud(tmp_path / "missing" / "cloud.xyz", surfaces)


# ----------------------------------------------------------------------------------------------------- the textured OBJ
def _arrays(s):
    a = s.arrays()
    return a["vertices"], a["edges"]


def _obj_surfaces(which):
    tall = lambda s: s.set_heights(np.sin(s.arrays()["vertices"][:, 0] / 9.0) * 3.0 + 101.37)
    if which == "minimal":
        return [tall(M.mesh("minimal"))]
    if which == "refined":
        return [M.mesh("refined1")]
    if which == "two":
        return [tall(M.mesh("grid3x3")), M.mesh("refined0")]
    no_edges = host.Surface().set(np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]), np.zeros((0, 5), np.uint64))
    return [M.mesh("minimal"), no_edges, tall(M.mesh("grid4x3"))]


@pytest.mark.parametrize("which", ["minimal", "refined", "two", "skipped"])
def test_textured_obj_equals_the_yardstick(which):
    surfaces = _obj_surfaces(which)
    obj, mtl = host.textured_obj(surfaces, GEOMETRY, "survey")
    yard_obj, yard_mtl = F.driver_obj([_arrays(s) for s in surfaces], GEOMETRY, "survey")
    assert mtl == yard_mtl == (b"newmtl orthomosaic_material\nKa 1.0 1.0 1.0\nKd 1.0 1.0 1.0\nKs 0.0 0.0 0.0\nmap_Kd survey.jpg\n")
    assert obj == yard_obj
    lines = yard_obj.split(b"\n")
    assert lines[:2] == [b"mtllib survey.mtl", b"usemtl orthomosaic_material"]
    with_edges = [s for s in surfaces if len(s.arrays()["edges"])]
    n_vertices = sum(len(s.arrays()["vertices"]) for s in with_edges)
    assert sum(l.startswith(b"v ") for l in lines) == sum(l.startswith(b"vt ") for l in lines) == n_vertices
    corners = [int(c.split(b"/")[0]) for l in lines if l.startswith(b"f ") for c in l.split()[1:]]
    assert min(corners) == 1 and max(corners) == n_vertices      # the offset: the last surface reaches the last vertex
    if which == "skipped":
        assert len(with_edges) == 2 and b"v 1 2 3" not in yard_obj
    x, y, _ = with_edges[0].arrays()["vertices"][0]
    u, v = (x - GEOMETRY[2]) / (GEOMETRY[0] * GEOMETRY[4]), 1.0 - (GEOMETRY[3] - y) / (GEOMETRY[1] * GEOMETRY[5])
    assert lines[3] == b"vt %g %g" % (u, v)


@pytest.mark.parametrize("name", ["minimal", "grid4x3", "refined2"])
def test_obj_faces_are_the_ply_writers(name, tmp_path):
    s = M.mesh(name)
    s.save_ply(tmp_path / "mesh.ply")
    ply = (tmp_path / "mesh.ply").read_text().split("\n")
    count = lambda what: int([l for l in ply if l.startswith("element %s " % what)][0].split()[2])
    rows = ply[ply.index("end_header") + 1:]
    n_faces = count("face")
    ply_faces = [tuple(int(w) for w in l.split()[1:]) for l in rows[count("vertex"):count("vertex") + n_faces]]
    assert all(l.startswith("3 ") for l in rows[count("vertex"):count("vertex") + n_faces])
    obj, _ = host.textured_obj([s], GEOMETRY, "m")
    obj_faces = [tuple(int(c.split(b"/")[0]) - 1 for c in l.split()[1:]) for l in obj.split(b"\n") if l.startswith(b"f ")]
    assert all(c.split(b"/")[0] == c.split(b"/")[1] for l in obj.split(b"\n") if l.startswith(b"f ") for c in l.split()[1:])
    assert obj_faces == ply_faces and len(obj_faces) == n_faces == len(M.triangles(s))


def test_save_textured_obj_takes_the_geometry_from_the_plan(tmp_path):
    surfaces = _obj_surfaces("two")
    plan = dict(width=GEOMETRY[0], height=GEOMETRY[1], gsd=GEOMETRY[4], min_x=GEOMETRY[2], max_x=11.244, min_y=65.442,
                max_y=GEOMETRY[3], mean_camera_z=50.0)
    rgba = np.random.default_rng(0).integers(0, 256, (plan["height"], plan["width"], 4), dtype=np.uint8)
    texture = host.save_textured_obj(tmp_path / "site.obj", surfaces, rgba, plan)
    assert texture.shape == (480, 640, 3) and np.array_equal(texture, rgba[:, :, :3])
    obj, mtl = host.textured_obj(surfaces, GEOMETRY, "site")
    assert (tmp_path / "site.obj").read_bytes() == obj and (tmp_path / "site.mtl").read_bytes() == mtl
    assert sorted(os.listdir(tmp_path)) == ["site.mtl", "site.obj"]
    assert host.save_textured_obj(None, surfaces, rgba, plan)[:2] == host.textured_obj(surfaces, plan, "model")
    with pytest.raises(ValueError):
        host.save_textured_obj(None, surfaces, rgba[:10], plan)

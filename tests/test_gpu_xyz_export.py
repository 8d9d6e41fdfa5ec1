"""The point cloud file on the device (csrc/xyz_export.hip) against the host route of the same
library, which runs the same header (csrc/xyz_export.hpp) in host loops and is itself held against the yardstick program and
'%g' by test_xyz_export_host.py.  Byte for byte and integer for integer."""
import numpy as np
import pytest

import xyz_export_fixtures as F
from opencalibration_amd import capi, host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _device(ctx, xyz, bounds):
    e = capi.XyzExport(ctx, xyz)
    try:
        return e.text(bounds), e.kept
    finally:
        e.close()


def _sized_cloud(n, seed):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(-150, 150, n), rng.uniform(-150, 150, n), rng.normal(-48, 2.0, n)])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 140_000])
def test_sizes_across_wavefront_workgroup_and_scan_block_edges(ctx, n):
    """0, 1, a wavefront less one, one, one and a lane, a workgroup and a lane, and 2 x 70 000 points in two clouds (many
    workgroups, several blocks of the scan)."""
    xyz = _sized_cloud(n, n)
    e = capi.XyzExport(ctx, xyz)
    assert e.n == n
    box = e.bounds()
    assert box == host.cloud_outlier_bounds(xyz)
    for bounds in (box, None):
        text, kept = host.cloud_to_xyz(xyz, bounds=bounds, want_kept=True)
        assert e.text(bounds) == text and e.kept == kept
    e.close()
    if n == 140_000:
        surfaces = [host.Surface().set_clouds([xyz[:70_000], xyz[70_000:]])]
        assert host.cloud_outlier_bounds(surfaces, ctx=ctx) == box
        assert host.cloud_to_xyz(surfaces, ctx=ctx) == host.cloud_to_xyz(surfaces)


def test_lines_of_every_length(ctx):
    """6 bytes (0,0,0), the longest line the integer formatter writes - three negative scientific numbers of 12 characters,
    two commas and the newline: 39 bytes -, lengths between, and the two extremes mixed inside one workgroup."""
    short, long_ = [0.0, 0.0, 0.0], [-1.23457e-5, -9.87654e17, -3.33333e-5]
    ladder = [[0.0, 0.0, v] for v in (1.0, -1.0, 1.5, -1.5, 1.25, -1.25, 1.125, -1.125, 1.0625, -1.0625, 1.03125, -1.03125, -1.23456e10, -1.23456e-5)]
    rng = np.random.default_rng(1)
    mixed = [long_ if k else short for k in rng.integers(0, 2, 256)]
    xyz = np.array([short] * 70 + [long_] * 70 + ladder + mixed + [short, long_] * 200)
    expected = host.cloud_to_xyz(xyz, bounds=None)
    lengths = {len(l) + 1 for l in expected.split(b"\n")[:-1]}
    assert min(lengths) == 6 and max(lengths) == 39 and len(lengths) >= 10
    assert expected.startswith(b"0,0,0\n") and b"-1.23457e-05,-9.87654e+17,-3.33333e-05\n" in expected
    assert _device(ctx, xyz, None) == (expected, len(xyz))


def test_three_fallback_coordinates_in_the_middle(ctx):
    xyz = _sized_cloud(1000, 5)
    xyz[400, 0], xyz[401, 1], xyz[700, 2] = 1e-7, -1.7976931348623157e308, 5e-324
    expected = host.cloud_to_xyz(xyz, bounds=None)
    assert b"1e-07," in expected and b",-1.79769e+308," in expected and b",4.94066e-324\n" in expected
    assert _device(ctx, xyz, None) == (expected, 1000)
    box = ((-140, 140), (-140, 140), (-60, -40))               # two of the three lines are outside the box
    assert _device(ctx, xyz, box) == host.cloud_to_xyz(xyz, bounds=box, want_kept=True)


@pytest.mark.parametrize("name", list(F.cloud_cases()))
def test_every_bounds_case_of_the_host_test(ctx, name):
    case = F.cloud_cases()[name]
    xyz, surfaces = F.flat(case), F.surfaces_of(case)
    box = host.cloud_outlier_bounds(surfaces)
    assert host.cloud_outlier_bounds(surfaces, ctx=ctx) == box
    for bounds in ("filter", None, F.CUSTOM_BOX, ((0, 0),) * 3):
        assert host.cloud_to_xyz(surfaces, bounds=bounds, ctx=ctx, want_kept=True) == host.cloud_to_xyz(surfaces, bounds=bounds, want_kept=True)
    e = capi.XyzExport(ctx, xyz)
    assert e.bounds() == box and e.text(box) == host.cloud_to_xyz(xyz, bounds=box)
    e.close()


def test_save_pointcloud_on_the_device(ctx, tmp_path):
    surfaces = F.surfaces_of(F.cloud_cases()["two_by_two"])
    assert host.save_pointcloud(tmp_path / "device.xyz", surfaces, ctx=ctx) == host.save_pointcloud(tmp_path / "host.xyz", surfaces)
    assert (tmp_path / "device.xyz").read_bytes() == (tmp_path / "host.xyz").read_bytes() != b""


def test_export_from_mesh_points_handles(ctx):
    import mesh_points_fixtures as M

    s = M.mesh("grid3x3")
    clouds = M.clouds_for(s)["two"]
    points = [capi.MeshPoints(ctx, c) for c in clouds]
    table = s.locate_table()
    before = [p.count(table) for p in points]
    both = np.concatenate(clouds)
    from_points, from_host = capi.XyzExport.from_points(ctx, points), capi.XyzExport(ctx, both)
    assert from_points.n == from_host.n == len(both)
    assert from_points.bounds() == from_host.bounds() == host.cloud_outlier_bounds(both)
    for bounds in (from_host.bounds(), None):
        assert from_points.text(bounds) == from_host.text(bounds) == host.cloud_to_xyz(both, bounds=bounds)
    swapped = capi.XyzExport.from_points(ctx, points[::-1])
    assert swapped.text(None) == host.cloud_to_xyz(np.concatenate(clouds[::-1]), bounds=None)
    for p, b in zip(points, before):                           # the handles still count as they did
        after = p.count(table)
        assert all(np.array_equal(after[k].view(np.uint8), b[k].view(np.uint8)) for k in b)
    points[0].close()
    assert from_points.text(None) == from_host.text(None)      # the export holds its own copy
    with pytest.raises(capi.OchipError, match="not a live ochip_mesh_points"):
        capi.XyzExport.from_points(ctx, [points[1], points[0].raw])
    for x in (points[1], from_points, from_host, swapped):
        x.close()


def test_one_export_queried_twice(ctx):
    xyz = F.survey_cloud()
    e = capi.XyzExport(ctx, xyz)
    box = e.bounds()
    first, all_ = e.text(box), e.text(None)
    assert e.bounds() == box and e.text(box) == first != all_ and e.text(None) == all_
    assert first == host.cloud_to_xyz(xyz) and all_ == host.cloud_to_xyz(xyz, bounds=None)
    e.close()


def test_refusals(ctx):
    xyz = F.survey_cloud(300, 5)
    e = capi.XyzExport(ctx, xyz)
    nbytes, kept = e.text_size(None)
    assert kept == len(xyz)
    with pytest.raises(capi.OchipError, match="room for"):
        e.text(None, cap=nbytes - 1)
    assert e.text(None, cap=nbytes + 7) == host.cloud_to_xyz(xyz, bounds=None)
    e.close()
    e.close()                                                  # a second destroy is nothing
    for call in (lambda: e.bounds(handle=e.raw), lambda: e.text_size(None, handle=e.raw)):
        with pytest.raises(capi.OchipError, match="not a live ochip_xyz_export"):
            call()
    assert ctx.L.ochip_xyz_export_size(e.raw) == 0
    fresh = capi.XyzExport(ctx, xyz)
    rc = ctx.L.ochip_xyz_export_text(fresh.h, None, 0)         # text before any text_size
    assert rc != 0 and b"text_size has not run" in ctx.L.ochip_last_error(ctx.h)
    assert ctx.L.ochip_xyz_export_bounds(fresh.h, None) != 0 and b"NULL" in ctx.L.ochip_last_error(ctx.h)
    fresh.close()
    for bad in (np.nan, np.inf, -2.0 ** 63):
        broken = xyz.copy()
        broken[211, 2] = bad
        b = capi.XyzExport(ctx, broken)
        with pytest.raises(capi.OchipError, match="not finite or not below 2\\^63"):
            b.bounds()
        b.close()
        with pytest.raises(capi.OchipError, match="not finite or not below 2\\^63"):
            host.cloud_to_xyz(broken, ctx=ctx)


def test_format_g6_on_the_device_over_the_million_values(ctx):
    v = F.number_family()
    text, length = ctx.format_g6(v)
    host_text, host_length = host.format_g6(v, fallback=False)
    assert np.array_equal(text, host_text) and np.array_equal(length, host_length) and (length > 0).all()
    declined, declined_length = ctx.format_g6(F.FALLBACK_VALUES + [np.nan, np.inf])
    assert (declined_length == 0).all() and (declined == b"").all()

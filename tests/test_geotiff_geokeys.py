"""The GeoKeys of the survey's local frame: a GeoTIFF written with geo["origin"] or geo["coord"] carries
the user-defined Transverse Mercator in tags 34735 / 34736 / 34737, GeoTiffReader.projection reads it back, and a file
written with an EPSG code is, byte for byte, what the writer gave before the keys existed."""
import hashlib
import io
import struct

import numpy as np
import pytest

from opencalibration_amd import host

PIL = pytest.importorskip("PIL.Image")

TABLE = [(1024, 1), (1025, 1), (1026, "Custom Transverse Mercator"), (2048, 4326), (2049, "WGS 84"), (2054, 9102), (3072, 32767),
         (3074, 32767), (3075, 1), (3076, 9001), (3080, "lon"), (3081, "lat"), (3082, 0.0), (3083, 0.0), (3092, 1.0)]
# sha256 of save_geotiff(raster(), geo=dict(min_x=100.5, max_y=2000.25, gsd=0.05, epsg=32633)) on the CPU route by the
# writer of the commit before this one
EPSG_FILE_SHA256 = "d6bd792a680dfb7024f1835ad5685acdf0972592ddd62f343fcba3d02a2af99f"


def raster():
    y, x = np.mgrid[0:70, 0:90]
    return np.stack([(x * 3) % 256, (y * 5) % 256, (x + y) % 256, np.where((x + y) % 7 == 0, 0, 255)], -1).astype(np.uint8)


def written(geo, **kw):
    out = io.BytesIO()
    host.save_geotiff(out, raster(), geo=geo, **kw)
    return out.getvalue()


def decode_keys(data):
    """[(key, value)] of the GeoKey directory as Pillow reads tags 34735 / 34736 / 34737; doubles stay bit patterns"""
    tags = PIL.open(io.BytesIO(data)).tag_v2
    directory, doubles, text = tags[34735], tags.get(34736, ()), tags.get(34737, "")
    assert tuple(directory[:3]) == (1, 1, 0) and len(directory) == 4 + 4 * directory[3]
    out = []
    for q in range(directory[3]):
        key, loc, count, value = directory[4 + 4 * q:8 + 4 * q]
        if loc == 0:
            assert count == 1
            out.append((key, value))
        elif loc == 34736:
            assert count == 1
            out.append((key, struct.pack("<d", doubles[value])))
        else:
            assert loc == 34737 and text[value + count - 1] == "|"
            out.append((key, text[value:value + count - 1]))
    return out, text


@pytest.mark.parametrize("how", ["origin", "coord"])
@pytest.mark.parametrize("lat, lon", [(47.376912, 151.234567), (-33.9, 18.4)])
def test_the_key_table_and_the_origin_doubles(how, lat, lon):
    coord = host.GeoCoord(lat, lon)
    geo = dict(min_x=-12.5, max_y=40.25, gsd=0.125)
    geo[how] = (lat, lon) if how == "origin" else coord
    data = written(geo)
    keys, text = decode_keys(data)
    assert [k for k, _ in keys] == sorted(k for k, _ in keys)                       # ascending
    want = []
    for key, value in TABLE:                                                        # the rounded pair, bit for bit
        value = {"lon": coord.centre[1], "lat": coord.centre[0]}.get(value, value) if isinstance(value, str) else value
        want.append((key, struct.pack("<d", value) if isinstance(value, float) else value))
    assert keys == want
    assert text.rstrip("\0") == "Custom Transverse Mercator|WGS 84|"
    assert coord.centre == (float("%g" % lat), float("%g" % lon))
    with host.GeoTiffReader(data) as rd:
        assert rd.projection == dict(kind="tmerc", lat0=coord.centre[0], lon0=coord.centre[1], k0=1.0, false_easting=0.0,
                                     false_northing=0.0)
        assert rd.geo == dict(min_x=-12.5, max_y=40.25, gsd_x=0.125, gsd_y=0.125, epsg=32767)   # its five keys, user-defined
        assert np.array_equal(rd.read(), raster())


def test_the_float_raster_and_bigtiff_carry_them_too():
    dsm = np.linspace(0, 1, 40 * 30, dtype=np.float32).reshape(40, 30)
    for big in (False, True):
        out = io.BytesIO()
        host.save_geotiff(out, dsm, geo=dict(min_x=0.0, max_y=0.0, gsd=1.0, origin=(10.0, 20.0)), bigtiff=big)
        with host.GeoTiffReader(out.getvalue()) as rd:
            assert rd.projection["lat0"] == 10.0 and rd.projection["lon0"] == 20.0
            assert np.array_equal(rd.read(), dsm)


def test_without_the_new_keys_nothing_changes():
    geo = dict(min_x=100.5, max_y=2000.25, gsd=0.05, epsg=32633)
    data = written(geo)
    assert hashlib.sha256(data).hexdigest() == EPSG_FILE_SHA256
    keys, _ = decode_keys(data)
    assert keys == [(1024, 1), (1025, 1), (3072, 32633)]
    with host.GeoTiffReader(data) as rd:
        assert rd.projection is None
        assert rd.geo == dict(min_x=100.5, max_y=2000.25, gsd_x=0.05, gsd_y=0.05, epsg=32633)
    with host.GeoTiffReader(written(dict(min_x=0.0, max_y=1.0, gsd=2.0))) as rd:
        assert rd.projection is None and rd.geo["epsg"] is None
    with host.GeoTiffReader(written(None)) as rd:
        assert rd.projection is None and rd.geo is None


def test_a_frame_and_an_epsg_code_together_are_refused():
    with pytest.raises(ValueError):
        written(dict(min_x=0.0, max_y=0.0, gsd=1.0, epsg=32633, origin=(1.0, 2.0)))

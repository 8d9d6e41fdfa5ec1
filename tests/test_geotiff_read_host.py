"""Reading tiled DEFLATE GeoTIFFs on the host route (csrc/inflate_rules.hpp, csrc/host/geotiff_read.cpp, host.GeoTiffReader;
DESIGN.md section 4.21): the inflate against zlib, the hand-assembled corners, the refusals, the reader against the arrays
the files were built from, and the stand-alone program under the sanitizers."""
import io
import warnings
import zlib

import numpy as np
import pytest

import geotiff_fixtures as G
import geotiff_read_fixtures as R
import mesh_points_fixtures as M
from opencalibration_amd import host

OK, CORRUPT = host.INFLATE_OK, host.INFLATE_CORRUPT


def _check_zoo(zoo, ctx=None):
    report = host.inflate_report([z for _, z, _ in zoo], [len(d) for _, _, d in zoo], ctx=ctx)
    for (name, _, data), (status, produced, got) in zip(zoo, report):
        assert status == OK and produced == len(data) and got == data, name


# ---------------------------------------------------------------------------------------------------------------- the inflate
def test_inflate_gives_what_zlib_gives():
    zoo = R.zoo()
    for name, z, data in zoo[::37]:
        assert zlib.decompress(z) == data, name
    _check_zoo(zoo)
    assert host.inflate_streams([z for _, z, _ in zoo[:40]], [len(d) for _, _, d in zoo[:40]]) == [d for _, _, d in zoo[:40]]
    assert host.inflate_streams([], 5) == []


def test_inflate_hand_assembled_cases():
    for name, (z, data) in R.hand_cases().items():
        assert host.inflate_streams([z], len(data)) == [data], name


def test_inflate_takes_this_projects_own_streams():
    names, payloads = G.crafted()
    noise = np.random.default_rng(3).integers(0, 256, (1, G.PAYLOAD), dtype=np.uint8)
    payloads = np.concatenate([payloads, noise])
    streams = host.deflate_tiles(payloads)
    assert len(streams[-1]) == host.GEOTIFF_MAX_STREAM                     # the stored 17-block fallback
    got = host.inflate_streams(streams, G.PAYLOAD)
    for k, g in enumerate(got):
        assert g == payloads[k].tobytes(), k


def test_inflate_refuses_what_the_rules_refuse():
    cases = R.refusals()
    report = host.inflate_report([z for z, _ in cases.values()], [e for _, e in cases.values()])
    for name, (status, produced, got) in zip(cases, report):
        assert status == CORRUPT and got is None, name
    z, expect = cases["wrong_adler"]
    good = zlib.compress(b"abc")
    with pytest.raises(host.GeoTiffError, match="stream 1 of 3") as e:
        host.inflate_streams([good, z, good], [3, expect, 3])
    assert e.value.status == "corrupt"


def test_inflate_truncated_at_every_byte_and_mutated():
    z, data = R.small_stream()
    cuts = [z[:k] for k in range(len(z))]
    for status, produced, got in host.inflate_report(cuts, len(data)):
        assert status == CORRUPT and got is None and produced <= len(data)
    muts = R.mutations(z, 400, seed=1) + R.mutations(zlib.compress(R.payload("ramp", 5000), 9), 400, seed=2)
    expects = [len(data)] * 400 + [5000] * 400
    accepted = 0
    for m, expect, (status, produced, got) in zip(muts, expects, host.inflate_report(muts, expects)):
        ref, ok = R.inflate_by_zlib(m)
        if ok and len(ref) == expect:
            assert status == OK and got == ref
            accepted += 1
        else:
            assert status == CORRUPT and got is None
    assert accepted < 100


def test_inflate_argument_refusals():
    with pytest.raises(ValueError, match="2 streams and 1 sizes"):
        host.inflate_report([b"", b""], [1])
    L = host.load()
    rd = host._TileReader(1, False, 16, 16, 16, 16, 1, None)
    one = np.zeros(8, np.uint64)
    assert L.och_geotiff_reader_inflate(rd.h, 65536, None, None, None, None, 0, None, None) == -1
    assert "65535 streams" in rd._error()
    assert L.och_geotiff_reader_inflate(rd.h, 1, one.ctypes.data, None, None, None, 0, None, None) == -1
    assert "offsets are NULL" in rd._error()
    dead = rd.h
    rd.close()
    assert L.och_geotiff_reader_inflate(dead, 0, None, None, None, None, 0, None, None) == -1
    assert "not a live" in L.och_geotiff_read_last_error().decode()
    assert L.och_geotiff_reader_launches(dead) == -1
    L.och_geotiff_reader_destroy(dead)                          # a dead handle is refused, not followed
    assert L.och_geotiff_reader_inflate(None, 0, None, None, None, None, 0, None, None) == -1
    for bad in (dict(samples=2), dict(tile_w=24), dict(tile_w=2048, tile_h=1024), dict(predictor=3), dict(width=0), dict(is_float=True, samples=3)):
        kw = dict(samples=4, is_float=False, width=100, height=100, tile_w=16, tile_h=16, predictor=2)
        kw.update(bad)
        with pytest.raises(host.GeoTiffError) as e:
            host._TileReader(kw["samples"], kw["is_float"], kw["width"], kw["height"], kw["tile_w"], kw["tile_h"], kw["predictor"], None)
        assert e.value.status == "refused"


# ----------------------------------------------------------------------------------------------------------------- the reader
def _written(name, **kw):
    a = G.dsm() if name == "dsm" else G.rgba(name)
    f = io.BytesIO()
    host.save_geotiff(f, a, geo=G.GEO, **kw)
    return a, f.getvalue()


@pytest.mark.parametrize("name", G.RGBA + ("dsm",))
def test_reader_returns_what_the_writer_was_fed(name):
    for kw in (dict(bigtiff=False, sparse=True), dict(bigtiff=True, sparse=False), dict(bigtiff=False, sparse=False), dict(bigtiff=True, sparse=True)):
        a, data = _written(name, **kw)
        levels = host.ortho_overviews(a)
        with host.GeoTiffReader(data) as rd:
            assert (rd.width, rd.height) == (a.shape[1], a.shape[0]) and rd.big == kw["bigtiff"]
            assert rd.kind == (host.OVERVIEW_FLOAT32 if name == "dsm" else host.OVERVIEW_RGBA8) and rd.samples == (1 if name == "dsm" else 4)
            assert rd.levels == [tuple(l.shape[:2]) for l in levels]
            assert rd.geo == dict(min_x=G.GEO["min_x"], max_y=G.GEO["max_y"], gsd_x=G.GEO["gsd"], gsd_y=G.GEO["gsd"], epsg=G.GEO["epsg"])
            assert (rd.nodata is not None and np.isnan(rd.nodata)) if name == "dsm" else rd.nodata is None
            got = rd.read()
            assert got.dtype == a.dtype and got.tobytes() == a.tobytes()
            for k, l in enumerate(levels):
                assert rd.read(level=k + 1).tobytes() == np.ascontiguousarray(l).tobytes(), k
    raster, geo = host.load_geotiff(data, level=1 if levels else 0)
    assert raster.tobytes() == np.ascontiguousarray(levels[0] if levels else a).tobytes() and geo["epsg"] == G.GEO["epsg"]


SIZES = ((1, 1), (17, 33), (512, 512), (513, 511), (1100, 700))            # width x height
MATRIX = [(layout, predictor, tile, size) for layout in (1, 3, 4, "f") for predictor in (1, 2) for tile in (16, 48, 512) for size in SIZES]


def _windows(h, th):
    w = {(0, h), (h - 1, 1), (0, 1)}
    if h > 3:
        w.add((1, min(th, h) - 2 if min(th, h) > 3 else 1))               # inside one tile row
    if h > th:
        w |= {(th - 1, 2), ((h - 1) // th * th, h - (h - 1) // th * th)}  # across a tile-row boundary; the last partial block
    return sorted(w)


@pytest.mark.parametrize("layout, predictor, tile, size", MATRIX)
def test_reader_over_the_taken_matrix(layout, predictor, tile, size):
    k = MATRIX.index((layout, predictor, tile, size))
    w, h = size
    a = R.raster(layout, h, w)
    if k % 3 == 0 and layout != "f":
        a = a.copy()
        a[:, : w // 2] = 0                                                  # whole tiles of zeros, for the sparse variant
    data = R.build_tiff(a, tile=(tile, tile), big=k % 2 == 1, predictor=predictor, compression=(8, 32946)[k // 2 % 2],
                        level=(6, 1, 9, 0)[k % 4], sparse=k % 3 == 0)
    with host.GeoTiffReader(io.BytesIO(data)) as rd:
        assert (rd.width, rd.height, rd.samples) == (w, h, 1 if layout == "f" else layout) and rd.geo is None and rd.levels == []
        for row0, rows in _windows(h, tile):
            got = rd.read(row0, rows)
            assert got.shape == a[row0:row0 + rows].shape and got.tobytes() == a[row0:row0 + rows].tobytes(), (row0, rows)
        out = np.zeros_like(a[:h // 2])
        assert rd.read(0, h // 2, out=out) is out and out.tobytes() == a[:h // 2].tobytes()


def test_reader_takes_rectangular_tiles_levels_and_a_path(tmp_path):
    a = R.raster(4, 100, 150)
    levels = [a, a[::2, ::2].copy(), a[::4, ::4].copy()]
    geo = dict(min_x=-5.5, max_y=77.25, gsd_x=0.5, gsd_y=0.25, epsg=None)
    (tmp_path / "r.tif").write_bytes(R.build_tiff(levels, tile=(64, 32), geo=geo, nodata="-9999"))
    with host.GeoTiffReader(tmp_path / "r.tif") as rd:
        assert rd.levels == [(50, 75), (25, 38)] and rd.geo == geo and rd.nodata == -9999.0
        for k, l in enumerate(levels):
            assert rd.read(level=k).tobytes() == l.tobytes()
        with pytest.raises(ValueError):
            rd.read(90, 11)
        with pytest.raises(ValueError):
            rd.read(level=3)
        with pytest.raises(ValueError):
            rd.read(on_device=True)
        with pytest.raises(ValueError):
            rd.read(out=np.zeros((100, 150, 3), np.uint8))
    with pytest.raises(host.GeoTiffError, match="closed"):
        rd.read()


def test_pillow_reads_the_builders_files():
    Image = pytest.importorskip("PIL.Image")
    for layout in (4, "f"):
        a = R.raster(layout, 70, 90)
        if layout == "f":
            a = np.nan_to_num(a)
        with Image.open(io.BytesIO(R.build_tiff(a, tile=(32, 48)))) as im:
            assert np.array_equal(np.asarray(im), a)


UNSUPPORTED = {
    "big-endian": dict(byte_order=b"MM"), "strips": dict(drop=(322, 323, 324, 325), override={273: (4, [8]), 278: (4, [16]), 279: (4, [10])}),
    "compression 1": dict(compression=1), "compression 5": dict(compression=5), "Predictor 3": dict(override={317: (3, [3])}),
    "PlanarConfiguration 2": dict(override={284: (3, [2])}), "16": dict(override={258: (3, [16] * 4)}),
    "SampleFormat 2": dict(override={339: (3, [2] * 4)}), "tiles of 24": dict(override={322: (3, [24])}),
    "2 samples": dict(override={277: (3, [2]), 258: (3, [8, 8]), 339: (3, [1, 1])}),
}


@pytest.mark.parametrize("reason", sorted(UNSUPPORTED))
def test_unsupported_files_say_why(reason):
    data = R.build_tiff(R.raster(4, 40, 40), tile=(16, 16), **UNSUPPORTED[reason])
    with pytest.raises(host.GeoTiffError, match=reason) as e:
        host.GeoTiffReader(data)
    assert e.value.status == "unsupported"


def test_corrupt_structures_and_tiles():
    a = R.raster(4, 40, 40)
    good = R.build_tiff(a, tile=(16, 16))
    cases = {
        "IFD chain returns": R.build_tiff(a, tile=(16, 16), next_of_last=True),
        "outside the file": R.build_tiff(a, tile=(16, 16), next_of_last=1 << 30),
        "tile offsets and": R.build_tiff(a, tile=(16, 16), override={325: (4, [5] * 8)}),
        "tile 2 at": R.build_tiff(a, tile=(16, 16), override={325: (4, [20, 20, 1 << 28] + [20] * 6)}),
        "tag 256 is missing": R.build_tiff(a, tile=(16, 16), drop=(256,)),
        "not a TIFF header": b"II*\x01" + good[4:],
        "the header": good[:6],
        "an IFD": good[:-20],
    }
    for text, data in cases.items():
        with pytest.raises(host.GeoTiffError, match=text) as e:
            host.GeoTiffReader(data)
        assert e.value.status == "corrupt", text
    with pytest.raises(host.GeoTiffError, match="path, bytes or a seekable"):
        host.GeoTiffReader(12)
    with pytest.raises(host.GeoTiffError, match="tag 325's values are not unsigned integers") as e:
        host.GeoTiffReader(R.build_tiff(a, tile=(16, 16), override={325: (2, b"123456789")}))
    assert e.value.status == "corrupt"
    with pytest.raises(host.GeoTiffError, match="tag 324's values are not unsigned integers"):
        host.GeoTiffReader(R.build_tiff(a, tile=(16, 16), override={324: (12, [1.5] * 9)}))
    f = io.BytesIO()
    f.write(good)                                                                    # the position is left at the end
    with host.GeoTiffReader(f) as rd:
        assert rd.read().tobytes() == a.tobytes()
    # a tile whose stream does not check: the error names the level and the tile, and nothing is returned
    with host.GeoTiffReader(good) as rd:
        at = int(rd._ifds[0]["offsets"][4]) + int(rd._ifds[0]["counts"][4]) - 1      # tile (1, 1)'s Adler-32
    bad = bytearray(good)
    bad[at] ^= 1
    with host.GeoTiffReader(bytes(bad)) as rd:
        assert rd.read(0, 16).tobytes() == a[:16].tobytes()                          # tile row 0 is whole
        out = np.zeros_like(a)
        with pytest.raises(host.GeoTiffError, match=r"level 0, tile \(1, 1\)") as e:
            rd.read(out=out)
        assert e.value.status == "corrupt"
    levels = [a, a[::2, ::2].copy()]
    data = bytearray(R.build_tiff(levels, tile=(16, 16)))
    with host.GeoTiffReader(bytes(data)) as rd:
        data[int(rd._ifds[1]["offsets"][1]) + 3] ^= 0x40
    with host.GeoTiffReader(bytes(data)) as rd:
        with pytest.raises(host.GeoTiffError, match=r"level 1, tile \(1, 0\)"):
            rd.read(level=1)


def test_textured_obj_from_the_file_equals_the_one_from_the_mosaic(tmp_path):
    surfaces = [M.mesh("minimal")]
    plan = dict(width=64, height=48, gsd=0.0371, min_x=-12.5, max_x=-10.1256, min_y=81.4692, max_y=83.25, mean_camera_z=50.0)
    rgba = np.random.default_rng(0).integers(0, 256, (48, 64, 4), dtype=np.uint8)
    host.save_geotiff(tmp_path / "orthomosaic.tif", rgba, geo=dict(min_x=plan["min_x"], max_y=plan["max_y"], gsd=plan["gsd"], epsg=32632))
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir()
    for jpeg in (True, False):
        one = host.save_textured_obj(tmp_path / "a" / "site.obj", surfaces, rgba, plan, jpeg=jpeg)
        two = host.save_textured_obj_from_geotiff(tmp_path / "b" / "site.obj", surfaces, tmp_path / "orthomosaic.tif", jpeg=jpeg)
        assert np.array_equal(one, two) if not jpeg else one == two
        for ext in ("obj", "mtl") + (("jpg",) if jpeg else ()):
            assert (tmp_path / "a" / f"site.{ext}").read_bytes() == (tmp_path / "b" / f"site.{ext}").read_bytes(), ext
    with pytest.raises(host.GeoTiffError, match="no geotransform"):
        host.save_textured_obj_from_geotiff(None, surfaces, R.build_tiff(rgba, tile=(16, 16)))


# ------------------------------------------------------------------------------------------ the program under the sanitizers
def test_the_stand_alone_program_under_the_sanitizers():
    """the whole zoo (the hand-assembled cases are part of it), the refusals, the truncations and the mutations of
    test_inflate_truncated_at_every_byte_and_mutated, and reader windows with ragged edges: the program ends clean and agrees
    with the library"""
    if not R.driver()[1]:
        warnings.warn("the sanitizer runtime does not link here: the stand-alone program ran without -fsanitize, memory safety unchecked")
    z, data = R.small_stream()
    streams = [(s, len(d)) for _, s, d in R.zoo()] + list(R.refusals().values()) + [(z[:k], len(data)) for k in range(len(z))] + \
        [(m, len(data)) for m in R.mutations(z, 400, seed=1)] + \
        [(m, 5000) for m in R.mutations(zlib.compress(R.payload("ramp", 5000), 9), 400, seed=2)] + [(z, len(data) - 1), (z, len(data) + 1)]
    jobs = [("I", s, e) for s, e in streams]
    readers = []
    for layout, predictor, tile, (w, h), window in ((4, 2, 16, (17, 33), (15, 3)), ("f", 2, 48, (513, 100), (0, 100)), (3, 2, 16, (50, 20), (19, 1)),
                                                     (1, 1, 32, (33, 65), (31, 34))):
        a = R.raster(layout, h, w)
        with host.GeoTiffReader(R.build_tiff(a, tile=(tile, tile), predictor=predictor, sparse=True)) as rd:
            lv = rd._ifds[0]
            ty0, ty1 = window[0] // tile, -(-(window[0] + window[1]) // tile)
            lo, hi = ty0 * lv["tiles_x"], ty1 * lv["tiles_x"]
            packed, offsets = host._pack_streams([rd.buf[int(o):int(o + c)].tobytes() for o, c in zip(lv["offsets"][lo:hi], lv["counts"][lo:hi])])
        want = a[window[0]:window[0] + window[1]].tobytes()
        readers.append(want)
        jobs.append(("R", (lv["samples"], lv["is_float"], w, h, tile, tile, predictor), window[0], window[1], packed[:int(offsets[-1])].tobytes(),
                     offsets))
    got = R.run_driver(jobs)
    report = host.inflate_report([s for s, _ in streams], [e for _, e in streams])
    assert got[:len(streams)] == report
    for (bad, raster), want in zip(got[len(streams):], readers):
        assert bad == -1 and raster == want

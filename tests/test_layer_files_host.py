"""The layers and cameras GeoTIFFs on the CPU route (csrc/deflate_rules.hpp, csrc/host/geotiff.cpp, host.GeoTiffWriter with
the kinds GEOTIFF_LAYERS8 and GEOTIFF_CAMERAS32; the reference's createMultiBandGeoTIFF,
src/ortho/ortho.cpp:969-1008).  The yardstick is outside the library: the reader of layer_files_fixtures.py walks the IFD,
inflates every tile with zlib.decompress, undoes the predictor with numpy's cumsum at the stride of the sample count and
de-interleaves; the comparison with the input is exact.  zlib's own Z_HUFFMAN_ONLY stream bounds the size.  Nothing loaded
into Python runs under a sanitizer: the host route is compiled into a stand-alone program (layer_files_driver.cpp) for that."""
import io
import os
import subprocess
import warnings
import zlib

import numpy as np
import pytest

import layer_files_fixtures as F
from opencalibration_amd import capi, host

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = [host.GEOTIFF_LAYERS8, host.GEOTIFF_CAMERAS32]


def raster_of(kind, content, w, h, L):
    return F.rasters(content, w, h, L)[KINDS.index(kind)]


def test_the_kinds_are_the_headers():
    assert (host.GEOTIFF_LAYERS8, host.GEOTIFF_CAMERAS32, host.GEOTIFF_MAX_LAYERS) == (F.LAYERS8, F.CAMERAS32, 2)
    for name, value in (("LAYERS8", 2), ("CAMERAS32", 3), ("MAX_LAYERS", 2)):
        text = open(os.path.join(os.path.dirname(HERE), "include", "ochip.h")).read()
        assert f"#define OCHIP_GEOTIFF_{name} {value}\n" in text


@pytest.mark.parametrize("content", F.CONTENTS)
@pytest.mark.parametrize("size", F.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("L", F.LAYERS)
@pytest.mark.parametrize("kind", KINDS)
def test_an_independent_reader_returns_the_input_however_it_is_fed(kind, L, size, content):
    w, h = size
    raster = raster_of(kind, content, w, h, L)
    data = F.written(host, kind, raster, geo=F.GEO)
    got, missing, sizes, _ = F.decode(data, kind, L)
    assert got.dtype == raster.dtype and got.shape == raster.shape and np.array_equal(got, raster)
    zero = [(ty, tx) for ty, tx, t in F.padded_tiles(kind, raster) if not t.any()]
    assert missing == zero  # sparse is the default: exactly the all-zero tiles are left out
    for step in F.STEPS[1:]:
        assert F.written(host, kind, raster, step, geo=F.GEO) == data, step


@pytest.mark.parametrize("kind", KINDS)
def test_sparse_leaves_out_exactly_the_all_zero_tiles(kind):
    raster = raster_of(kind, "layered", 1030, 520, 2)
    zero = [(ty, tx) for ty, tx, t in F.padded_tiles(kind, raster) if not t.any()]
    assert 0 < len(zero) < 6
    got, missing, _, _ = F.decode(F.written(host, kind, raster), kind, 2)
    assert missing == zero and np.array_equal(got, raster)
    got, missing, sizes, _ = F.decode(F.written(host, kind, raster, sparse=False), kind, 2)
    assert missing == [] and len(sizes) == 6 and np.array_equal(got, raster)
    # int64, as torch holds the ids, is the same file
    if kind == host.GEOTIFF_CAMERAS32:
        assert F.written(host, kind, raster.view(np.int64)) == F.written(host, kind, raster)


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("L", F.LAYERS)
@pytest.mark.parametrize("kind", KINDS)
def test_tags(kind, L, big):
    w, h = 513, 513
    raster = raster_of(kind, "layered", w, h, L)
    data = F.written(host, kind, raster, geo=F.GEO, bigtiff=big, sparse=False)
    ifds, is_big = F.P.parse(data)
    assert is_big == big and len(ifds) == 1  # no overview levels
    t = ifds[0]
    layers = kind == host.GEOTIFF_LAYERS8
    n = (4 if layers else 2) * L
    assert t[256] == (w,) and t[257] == (h,)
    assert t[258] == ((8,) * n if layers else (32,) * n)  # BitsPerSample
    assert t[259] == (8,)  # Compression: DEFLATE
    assert t[262] == (1,)  # Photometric: MINISBLACK
    assert t[277] == (n,)  # SamplesPerPixel
    assert t[284] == (1,)  # PlanarConfiguration: pixel interleave
    assert t[317] == (2,)  # Predictor
    assert t[322] == (512,) and t[323] == (512,) and len(t[324]) == len(t[325]) == 4
    assert t[338] == (0,) * (n - 1)  # ExtraSamples: unspecified
    assert t[339] == (1,) * n  # SampleFormat: unsigned
    assert t[33550] == (F.GEO["gsd"], F.GEO["gsd"], 0.0) and t[33922] == (0.0, 0.0, 0.0, F.GEO["min_x"], F.GEO["max_y"], 0.0)
    assert t[34735] == (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, F.GEO["epsg"])
    assert 254 not in t and 42113 not in t
    assert sorted(t) == [256, 257, 258, 259, 262, 277, 284, 317, 322, 323, 324, 325, 338, 339, 33550, 33922, 34735]
    assert 33550 not in F.P.parse(F.written(host, kind, raster))[0][0]
    # BigTIFF by the kind's own uncompressed size: 16 bytes a pixel cross the limit at a quarter of the 4-byte pixel's count
    assert host.geotiff_pixel_bytes(kind, L) == F.pixel_bytes(kind, L) == n * (1 if layers else 4)


def huffman_only(payload):
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
    return len(c.compress(payload) + c.flush())


@pytest.mark.parametrize("kind", KINDS)
def test_no_larger_than_zlib_huffman_only(kind):
    """At most 1.05 x zlib's own Huffman-only stream of the same payloads, the bound of
    test_geotiff_host.py::test_no_larger_than_zlib_huffman_only: the block cutting and the length limiter are the same rules,
    only the distances differ.  On the layered pattern at 513 x 513, L = 2, measured, the ratio to Huffman-only and to zlib
    level 6: layers 0.125 / 1.03, cameras 0.034 / 2.83."""
    raster = raster_of(kind, "layered", 513, 513, 2)
    data = F.written(host, kind, raster, sparse=False)
    _, _, sizes, _ = F.decode(data, kind, 2)
    payloads = [F.predict(t) for _, _, t in F.padded_tiles(kind, raster)]
    ours, theirs = sum(sizes), sum(map(huffman_only, payloads))
    six = sum(len(zlib.compress(p, 6)) for p in payloads)
    print("kind", kind, "ours", ours, "huffman-only", theirs, "level 6", six, "ratios", ours / theirs, ours / six)
    assert ours <= 1.05 * theirs


@pytest.mark.parametrize("L", F.LAYERS)
@pytest.mark.parametrize("kind", KINDS)
def test_noise_is_stored(kind, L):
    raster = raster_of(kind, "noise", 512, 512, L)
    _, missing, sizes, _ = F.decode(F.written(host, kind, raster), kind, L)
    payload = 512 * 512 * F.pixel_bytes(kind, L)
    assert missing == [] and sizes == [F.stored_bytes(payload)] == [host.geotiff_stored_bytes(payload)]


def test_payloads_of_the_kinds_own_size():
    """och_geotiff_payloads takes payloads of the kind's size: the stream of the test's own predicted payload is the tile's"""
    kind, L = host.GEOTIFF_CAMERAS32, 2
    raster = raster_of(kind, "layered", 512, 512, L)
    data = F.written(host, kind, raster)
    t = F.P.parse(data)[0][0]
    (_, _, tile), = F.padded_tiles(kind, raster)
    enc = host._TileEncoder(kind, 512, 512, None, True, num_layers=L)
    try:
        enc.payloads(np.frombuffer(F.predict(tile), np.uint8).reshape(1, -1))
        buf, counts = enc.collect()
        assert list(counts) == [t[325][0]] and buf.tobytes() == data[t[324][0]:t[324][0] + t[325][0]]
    finally:
        enc.close()


def test_refusals():
    bgra, ids = F.rasters("layered", 511, 3, 2)
    with pytest.raises(capi.OchipError, match="needs num_layers"):
        host.GeoTiffWriter(io.BytesIO(), host.GEOTIFF_LAYERS8, 511, 3)
    with pytest.raises(capi.OchipError, match="needs num_layers"):
        host.GeoTiffWriter(io.BytesIO(), host.GEOTIFF_CAMERAS32, 511, 3)
    with pytest.raises(capi.OchipError, match="num_layers belongs to"):
        host.GeoTiffWriter(io.BytesIO(), host.OVERVIEW_RGBA8, 511, 3, num_layers=2)
    for bad in (0, 3, -1, 2.0):
        with pytest.raises(capi.OchipError, match="num_layers is 1 .. 2"):
            host.GeoTiffWriter(io.BytesIO(), host.GEOTIFF_LAYERS8, 511, 3, num_layers=bad)
    with pytest.raises(capi.OchipError, match="0 x 3"):
        host.GeoTiffWriter(io.BytesIO(), host.GEOTIFF_LAYERS8, 0, 3, num_layers=2)
    # the library's own entry refuses the same, whoever calls it
    L = host.load()
    h = host.C.c_void_p()
    for kind, layers in ((host.GEOTIFF_LAYERS8, 3), (host.GEOTIFF_CAMERAS32, 0), (host.OVERVIEW_RGBA8, 1), (4, 1)):
        assert L.och_geotiff_create_layered(None, kind, layers, 8, 8, 1, host.C.byref(h)) == -1 and not h.value
        assert "och_geotiff_create_layered: kind 2 (layers) or 3 (cameras), 1 .. 2 layers" in L.och_geotiff_last_error().decode()
    assert L.och_geotiff_create(None, host.GEOTIFF_LAYERS8, 8, 8, 1, host.C.byref(h)) == -1  # the old entry keeps its two kinds
    assert "kind 0 (RGBA8) or 1 (float32)" in L.och_geotiff_last_error().decode()
    with host.GeoTiffWriter(io.BytesIO(), host.GEOTIFF_LAYERS8, 511, 3, num_layers=2) as wr:
        for band in (bgra[0], bgra[:1], bgra[:, :, :100], bgra[..., :3], ids, bgra.astype(np.int8), np.zeros((2, 3, 511), np.float32)):
            with pytest.raises(capi.OchipError, match=r"rows from 0: a band of this writer is \(2, rows, 511, 4\) uint8"):
                wr.feed(0, band)
        with pytest.raises(capi.OchipError, match=r"rows 1 \.\. 2 where row 0 is next \(a gap\)"):
            wr.feed(1, bgra[:, 1:2])
        wr.feed(0, bgra[:, :2])
        with pytest.raises(capi.OchipError, match=r"beyond the raster's 3"):
            wr.feed(2, bgra[:, :2])
        with pytest.raises(capi.OchipError, match=r"rows 2 \.\. 3 were never fed"):
            wr.finish()
    with host.GeoTiffWriter(io.BytesIO(), host.GEOTIFF_CAMERAS32, 511, 3, num_layers=2) as wr:
        for band in (ids[0], ids[:1], ids[:, :, :100], bgra, ids.astype(np.uint32), ids.astype(np.float64)):
            with pytest.raises(capi.OchipError, match=r"rows from 0: a band of this writer is \(2, rows, 511\) uint64 or int64"):
                wr.feed(0, band)
        wr.feed(0, ids)
        with pytest.raises(capi.OchipError, match="no overview levels"):
            wr.finish([ids])
        wr.finish()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("layer_files") / "driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unused-parameter", "-fopenmp", "-DOCHIP_GEOTIFF_READ_STANDALONE",
           "-o", exe, os.path.join(HERE, "layer_files_driver.cpp"),
           os.path.join(os.path.dirname(HERE), "opencalibration_amd", "csrc", "host", "geotiff_read.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        warnings.warn("the sanitizer runtimes do not link here: the driver runs plain")
        subprocess.run(cmd, check=True)
    return exe


def test_host_route_under_sanitizers(driver, tmp_path):
    """The host route over the fixture rasters in a stand-alone program built with -fsanitize=address,undefined: clean, and the
    same streams as the library gives Python"""
    jobs, want = [], []
    for k, (kind, L, (w, h), content, step) in enumerate([
            (host.GEOTIFF_LAYERS8, 2, (513, 513), "layered", 511), (host.GEOTIFF_CAMERAS32, 2, (513, 513), "layered", 7),
            (host.GEOTIFF_LAYERS8, 1, (1030, 520), "layered", 520), (host.GEOTIFF_CAMERAS32, 1, (511, 3), "noise", 1),
            (host.GEOTIFF_CAMERAS32, 2, (512, 512), "noise", 512), (host.GEOTIFF_LAYERS8, 2, (1, 1), "noise", 1),
            (host.GEOTIFF_LAYERS8, 2, (511, 3), "zero", 2)]):
        raster = raster_of(kind, content, w, h, L)
        rpath, spath = tmp_path / f"raster{k}.bin", tmp_path / f"streams{k}.bin"
        rpath.write_bytes(raster.tobytes())
        jobs.append((f"W {kind} {L} {w} {h} 1 {step} {rpath} {spath}", spath))
        data = F.written(host, kind, raster)
        t = F.P.parse(data)[0][0]
        want.append((list(t[325]), b"".join(data[o:o + c] for o, c in zip(t[324], t[325]))))
    (tmp_path / "list.txt").write_text("".join(j + "\n" for j, _ in jobs))
    r = subprocess.run([driver, str(tmp_path / "list.txt")], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(jobs)
    for line, (_, spath), (counts, streams) in zip(lines, jobs, want):
        fields = line.split()
        assert fields[0] == str(len(counts)) and [int(v) for v in fields[2:]] == counts, line
        assert spath.read_bytes() == streams


def test_reader_host_route_under_sanitizers(driver, tmp_path):
    """The reader's host route in the same program: good files in windows, then the damaged and truncated streams of the
    reader tests (geotiff_read_fixtures.mutations and cuts) in place of a tile - each names the tile or, where the damage
    leaves a valid stream of the same payload, returns the raster; the run is clean either way"""
    import geotiff_read_fixtures as R

    jobs = []  # (line, raster file, the expected raster or None, the tile that may be named)

    def job(kind, L, w, h, row0, rows, streams, expect, may_fail=None):
        k = len(jobs)
        offsets = np.zeros(len(streams) + 1, np.uint64)
        np.cumsum([len(z) for z in streams], out=offsets[1:])
        (tmp_path / f"s{k}.bin").write_bytes(b"".join(streams))
        (tmp_path / f"o{k}.bin").write_bytes(offsets.tobytes())
        jobs.append((f"R {kind} {L} {w} {h} {row0} {rows} {tmp_path / f's{k}.bin'} {tmp_path / f'o{k}.bin'} {tmp_path / f'r{k}.bin'}",
                     tmp_path / f"r{k}.bin", expect, may_fail))

    for kind, L, (w, h) in ((host.GEOTIFF_LAYERS8, 2, (513, 513)), (host.GEOTIFF_CAMERAS32, 2, (1030, 520)),
                            (host.GEOTIFF_CAMERAS32, 1, (511, 3)), (host.GEOTIFF_LAYERS8, 1, (1, 1))):
        raster = raster_of(kind, "layered", w, h, L)
        data = F.build_file(kind, raster)
        t = F.P.parse(data)[0][0]
        tiles_x = -(-w // 512)
        for row0, rows in WINDOWS:
            if row0 >= h:
                continue
            n = h - row0 if rows is None else min(rows, h - row0)
            ty0, ty1 = row0 // 512, -(-(row0 + n) // 512)
            streams = [data[o:o + c] for o, c in list(zip(t[324], t[325]))[ty0 * tiles_x:ty1 * tiles_x]]
            job(kind, L, w, h, row0, n, streams, raster[:, row0:row0 + n])
    kind, L, w, h = host.GEOTIFF_CAMERAS32, 2, 513, 3
    raster = np.ascontiguousarray(raster_of(kind, "layered", 513, 513, L)[:, 219:222])  # rows with ids in both tiles
    assert raster[:, :, :512].any() and raster[:, :, 512:].any()
    data = F.written(host, kind, raster, sparse=False)
    t = F.P.parse(data)[0][0]
    good = [data[o:o + c] for o, c in zip(t[324], t[325])]
    sparse = raster.copy()
    sparse[:, :, :512] = 0  # an empty stream is a sparse tile: tile 0 reads as zeros, tile 1 keeps its pixels
    job(kind, L, w, h, 0, 3, [b"", good[1]], sparse)
    for cut in (1, 2, 5, 6, len(good[0]) // 2, len(good[0]) - 4, len(good[0]) - 1):
        job(kind, L, w, h, 0, 3, [good[0][:cut], good[1]], None, 0)
    for z in R.mutations(good[0], 12, seed=7):
        job(kind, L, w, h, 0, 3, [z, good[1]], raster, 0)
    (tmp_path / "list.txt").write_text("".join(j[0] + "\n" for j in jobs))
    r = subprocess.run([driver, str(tmp_path / "list.txt")], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(jobs)
    named = 0
    for line, (_, rpath, expect, may_fail) in zip(lines, jobs):
        if line == "-1":
            assert expect is not None, "a truncated stream was taken"
            got = np.frombuffer(rpath.read_bytes(), expect.dtype).reshape(expect.shape)
            assert np.array_equal(got, expect), line
        else:
            assert may_fail is not None and line == str(may_fail), line
            named += 1
    assert named >= 12


# ---- the reader: GeoTiffReader's two layouts and read_layer_files, against files of the library and of zlib -----------------------
WINDOWS = [(0, None), (3, 1), (100, 300), (500, 20), (511, 2)]  # whole, and windows that start and end inside a tile row or cross one


def files_of(source, content, w, h, L):
    bgra, ids = F.rasters(content, w, h, L)
    if source == "ours":
        return bgra, ids, F.written(host, host.GEOTIFF_LAYERS8, bgra, geo=F.GEO), F.written(host, host.GEOTIFF_CAMERAS32, ids, geo=F.GEO)
    # the test's own writer: numpy's predictor, zlib at levels 1, 6, 9 and stored (level 0) tile by tile, sparse tiles left out
    return bgra, ids, F.build_file(F.LAYERS8, bgra, geo=F.GEO), F.build_file(F.CAMERAS32, ids, levels=(9, 0, 6, 1), geo=F.GEO, big=True)


@pytest.mark.parametrize("content", F.CONTENTS)
@pytest.mark.parametrize("size", F.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("L", F.LAYERS)
@pytest.mark.parametrize("source", ["ours", "zlib"])
def test_read_layer_files_returns_the_input(source, L, size, content):
    w, h = size
    bgra, ids, fl, fc = files_of(source, content, w, h, L)
    for row0, rows in WINDOWS:
        if row0 >= h:
            continue
        rows = None if rows is None else min(rows, h - row0)
        got = host.read_layer_files(fl, fc, row0, rows)
        n = h - row0 if rows is None else rows
        assert got["row0"] == row0 and got["rows"] == n
        assert got["bgra"].dtype == np.uint8 and got["bgra"].shape == (L, n, w, 4) and np.array_equal(got["bgra"], bgra[:, row0:row0 + n])
        assert got["camera_id"].dtype == np.uint64 and got["camera_id"].shape == (L, n, w)
        assert np.array_equal(got["camera_id"], ids[:, row0:row0 + n])


def test_the_reader_names_the_layouts():
    bgra, ids, fl, fc = files_of("zlib", "layered", 513, 513, 2)
    with host.GeoTiffReader(fl) as rd:
        assert (rd.kind, rd.num_layers, rd.samples, rd.width, rd.height, rd.levels) == (host.GEOTIFF_LAYERS8, 2, 8, 513, 513, [])
        assert rd.geo == dict(min_x=F.GEO["min_x"], max_y=F.GEO["max_y"], gsd_x=F.GEO["gsd"], gsd_y=F.GEO["gsd"], epsg=F.GEO["epsg"])
        assert np.array_equal(rd.read(), bgra)
        out = np.empty((2, 5, 513, 4), np.uint8)
        assert rd.read(508, 5, out=out) is out and np.array_equal(out, bgra[:, 508:513])
    with host.GeoTiffReader(fc) as rd:
        assert (rd.kind, rd.num_layers, rd.samples) == (host.GEOTIFF_CAMERAS32, 2, 4) and np.array_equal(rd.read(), ids)
    # one layer: the cameras file has two UInt32 samples; four Byte samples stay RGBA8, and read_layer_files reshapes them
    bgra, ids, fl, fc = files_of("ours", "layered", 513, 513, 1)
    with host.GeoTiffReader(fl) as rd:
        assert (rd.kind, rd.num_layers, rd.samples) == (host.OVERVIEW_RGBA8, None, 4) and np.array_equal(rd.read(), bgra[0])
    with host.GeoTiffReader(fc) as rd:
        assert (rd.kind, rd.num_layers, rd.samples) == (host.GEOTIFF_CAMERAS32, 1, 2) and np.array_equal(rd.read(), ids)


def test_a_damaged_tile_is_named_and_nothing_is_returned():
    bgra, ids, fl, fc = files_of("ours", "layered", 513, 513, 2)
    t = F.P.parse(fc)[0][0]
    bad = bytearray(fc)
    bad[t[324][0] + t[325][0] // 2] ^= 0x55
    with pytest.raises(host.GeoTiffError, match=r"corrupt: level 0, tile \(0, 0\): its stream is not a zlib stream of exactly 4194304 bytes"):
        host.read_layer_files(fl, bytes(bad))
    cut = fc[:t[324][0] + 40] + fc[t[324][0] + t[325][0]:]  # a truncated stream: the counts now reach into what follows
    with pytest.raises(host.GeoTiffError, match="corrupt"):
        host.read_layer_files(fl, cut)


def test_read_refusals():
    bgra, ids, fl, fc = files_of("ours", "layered", 513, 513, 2)
    with pytest.raises(host.GeoTiffError, match="refused: the cameras file holds no node ids"):
        host.read_layer_files(fl, fl)  # a layers file handed in as cameras
    with pytest.raises(host.GeoTiffError, match="refused: the layers file holds no B G R A layers"):
        host.read_layer_files(fc, fc)
    # one file of the pair alone
    with pytest.raises(host.GeoTiffError, match="refused: the layers file alone: the layers and the cameras file belong together"):
        host.read_layer_files(fl)
    with pytest.raises(host.GeoTiffError, match="refused: the layers file alone"):
        host.read_layer_files(fl, None)
    with pytest.raises(host.GeoTiffError, match="refused: the cameras file alone"):
        host.read_layer_files(None, fc)
    other = F.rasters("layered", 511, 3, 2)
    with pytest.raises(host.GeoTiffError, match="refused: the layers file is 513 x 513, the cameras file 511 x 3"):
        host.read_layer_files(fl, F.written(host, host.GEOTIFF_CAMERAS32, other[1], geo=F.GEO))
    one = F.rasters("layered", 513, 513, 1)
    with pytest.raises(host.GeoTiffError, match="refused: the layers file has 2 layers, the cameras file 1"):
        host.read_layer_files(fl, F.written(host, host.GEOTIFF_CAMERAS32, one[1], geo=F.GEO))
    with pytest.raises(host.GeoTiffError, match="refused: the layers file has 1 layers, the cameras file 2"):
        host.read_layer_files(F.written(host, host.GEOTIFF_LAYERS8, one[0], geo=F.GEO), fc)
    with pytest.raises(host.GeoTiffError, match="refused: the geo tags of the layers file"):
        host.read_layer_files(fl, F.written(host, host.GEOTIFF_CAMERAS32, ids, geo=dict(F.GEO, min_x=0.0)))
    with pytest.raises(host.GeoTiffError, match="refused: the geo tags of the layers file"):
        host.read_layer_files(fl, F.written(host, host.GEOTIFF_CAMERAS32, ids))
    # the library's entry
    L = host.load()
    h = host.C.c_void_p()
    for kind, layers in ((host.GEOTIFF_LAYERS8, 3), (host.GEOTIFF_CAMERAS32, 0), (host.OVERVIEW_RGBA8, 1)):
        assert L.och_geotiff_reader_create_layered(None, kind, layers, 8, 8, 16, 16, 2, 0, host.C.byref(h)) == -1 and not h.value
        assert "och_geotiff_reader_create_layered: the layers (kind 2) and cameras (kind 3) rasters have 1 or 2 layers" in \
            L.och_geotiff_read_last_error().decode()
    assert L.och_geotiff_reader_create_layered(None, host.GEOTIFF_CAMERAS32, 2, 8, 8, 1024, 512, 2, 0, host.C.byref(h)) == -1
    assert "a tile's payload is at most 4 MiB" in L.och_geotiff_read_last_error().decode()


# ---- the hand-over: the layer pass and the blend through the files ----------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    """the four-camera scene of test_color_balance_host.py::test_ortho_mosaic_solve_on_the_cpu_route, the solved mosaic without
    files and the bands ortho_layers gives: computed once"""
    from color_balance_fixtures import MOSAIC_CONFIG, MOSAIC_PLAN, smooth_images
    from layers_fixtures import four_camera_scene

    g, s, _ = four_camera_scene(seed=4)
    imgs = smooth_images(4, 120, 160)
    plan, cfg = dict(MOSAIC_PLAN), dict(MOSAIC_CONFIG)
    solved = host.ortho_mosaic(plan, g, [s], imgs, config=cfg, color_balance="solve")
    return g, s, imgs, plan, cfg, solved


def test_layers_files_then_blend_files_is_the_mosaic(scene, tmp_path):
    g, s, imgs, plan, cfg, _ = scene
    fl, fc, fd = tmp_path / "ortho.layers.tif", tmp_path / "ortho.cameras.tif", tmp_path / "dsm.tif"
    corr = host.ortho_layers_files(plan, g, [s], imgs, fl, fc, dsm_geotiff=fd, config=cfg)
    tables = host.color_balance_solve(corr, graph=g)
    want_file = io.BytesIO()
    want = host.ortho_mosaic(plan, g, [s], imgs, config=cfg, color_balance=tables, geotiff=want_file)
    got_file = io.BytesIO()
    got = host.ortho_blend_files(plan, g, [s], fl, fc, fd, color_balance=tables, config=cfg, geotiff=got_file)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    assert got_file.getvalue() == want_file.getvalue()
    # without tables as well
    assert np.array_equal(host.ortho_blend_files(plan, g, [s], fl, fc, fd, config=cfg), host.ortho_mosaic(plan, g, [s], imgs, config=cfg))
    # files that are not the plan's
    other = dict(plan, min_x=plan["min_x"] + 1.0)
    with pytest.raises(host.GeoTiffError, match="refused: the geo tags of the layers file"):
        host.ortho_blend_files(other, g, [s], fl, fc, fd, config=cfg)
    small = dict(plan, width=plan["width"] - 1)
    with pytest.raises(host.GeoTiffError, match="refused: the layers file is"):
        host.ortho_blend_files(small, g, [s], fl, fc, fd, config=cfg)
    with pytest.raises(host.GeoTiffError, match="refused: the cameras file holds no node ids"):
        host.ortho_blend_files(plan, g, [s], fl, fl, fd, config=cfg)


def test_the_solved_mosaic_with_the_files_is_the_one_without(scene):
    g, s, imgs, plan, cfg, solved = scene
    fl, fc = io.BytesIO(), io.BytesIO()
    got = host.ortho_mosaic(plan, g, [s], imgs, config=cfg, color_balance="solve", layers_geotiff=fl, cameras_geotiff=fc)
    assert np.array_equal(got, solved)
    # the two files hold ortho_layers' bands
    h, t = plan["height"], cfg.get("tile_size", host.LAYERS_CONFIG["tile_size"])
    lcfg = {k: v for k, v in cfg.items() if k in host.LAYERS_CONFIG}
    for row0 in range(0, h, t):
        rows = min(t, h - row0)
        dsm = host.dsm_render(plan, [s], row0=row0, rows=rows)
        lay = host.ortho_layers(plan, g, [s], imgs, row0=row0, tile_rows=1, config=lcfg, dsm=dsm)
        back = host.read_layer_files(fl.getvalue(), fc.getvalue(), row0, rows)
        assert np.array_equal(back["bgra"], lay["bgra"]) and np.array_equal(back["camera_id"], lay["camera_id"]), row0
    # the files of a single sweep - tables or none - are the same two
    f1, c1 = io.BytesIO(), io.BytesIO()
    plain = host.ortho_mosaic(plan, g, [s], imgs, config=cfg, layers_geotiff=f1, cameras_geotiff=c1)
    assert np.array_equal(plain, host.ortho_mosaic(plan, g, [s], imgs, config=cfg))
    assert f1.getvalue() == fl.getvalue() and c1.getvalue() == fc.getvalue()
    for one in (dict(layers_geotiff=io.BytesIO()), dict(cameras_geotiff=io.BytesIO())):
        with pytest.raises(capi.OchipError, match="layers_geotiff and cameras_geotiff belong together"):
            host.ortho_mosaic(plan, g, [s], imgs, config=cfg, **one)


def test_the_blend_reads_nothing_of_a_sample_whose_alpha_is_0(scene, tmp_path):
    """An invalid sample is colour 0, alpha 0, id 0 in the files the layer pass writes (ortho_layers.hpp's invalid sample, the
    reference's writeLayeredTileToGeoTIFF).  A file of another writer may hold anything there: the blend takes valid = alpha > 0
    and reads a sample's colour and looks up its id only when it is valid (ortho_blend.hpp, prep_pixel), so arbitrary colour
    and ids under alpha 0 give the same mosaic, bit for bit - through ortho_blend on the bands and through ortho_blend_files on
    files that zlib wrote"""
    g, s, imgs, plan, cfg, _ = scene
    fl, fc, fd = tmp_path / "ortho.layers.tif", tmp_path / "ortho.cameras.tif", tmp_path / "dsm.tif"
    corr = host.ortho_layers_files(plan, g, [s], imgs, fl, fc, dsm_geotiff=fd, config=cfg)
    tables = host.color_balance_solve(corr, graph=g)
    back = host.read_layer_files(fl, fc)
    bgra, ids = back["bgra"], back["camera_id"]
    hole = bgra[..., 3] == 0
    assert hole.any() and not hole.all() and hole[0].sum() != hole[1].sum()  # both kinds of sample, other holes per layer
    assert not bgra[hole].any() and not ids[hole].any()  # 0 / 0 / 0 as written
    assert ids[~hole].all()
    rng = np.random.default_rng(24)
    dirty_bgra, dirty_ids = bgra.copy(), ids.copy()
    dirty_bgra[hole, :3] = rng.integers(1, 256, (int(hole.sum()), 3), dtype=np.uint8)
    known = np.unique(ids[~hole])  # ids of real cameras as well as ids of none
    junk = rng.integers(1, 1 << 63, int(hole.sum()), dtype=np.uint64)
    junk[::2] = known[rng.integers(0, len(known), len(junk[::2]))]
    dirty_ids[hole] = junk
    assert dirty_bgra[hole, :3].all() and dirty_ids[hole].all() and not dirty_bgra[hole, 3].any()
    geo = dict(min_x=plan["min_x"], max_y=plan["max_y"], gsd=plan["gsd"], epsg=32632)
    dl, dc = F.build_file(F.LAYERS8, dirty_bgra, geo=geo), F.build_file(F.CAMERAS32, dirty_ids, geo=geo)
    for balance in (None, tables):
        want = host.ortho_blend_files(plan, g, [s], fl, fc, fd, color_balance=balance, config=cfg)
        assert want.any()
        assert np.array_equal(host.ortho_blend_files(plan, g, [s], dl, dc, fd, color_balance=balance, config=cfg), want)
        # and the blend itself, band by band
        bcfg = {k: v for k, v in cfg.items() if k in host.BLEND_CONFIG}
        t = cfg["tile_size"]
        for row0 in range(0, plan["height"], t):
            rows = min(t, plan["height"] - row0)
            dsm = host.dsm_render(plan, [s], row0=row0, rows=rows)
            lay = dict(bgra=np.ascontiguousarray(dirty_bgra[:, row0:row0 + rows]),
                       camera_id=np.ascontiguousarray(dirty_ids[:, row0:row0 + rows]), row0=row0, rows=rows)
            got = host.ortho_blend(plan, g, [s], lay, dsm, balance, config=bcfg)
            assert np.array_equal(got, want[row0:row0 + rows]), row0


def test_solve_refuses_a_file_object_it_cannot_read_back_before_it_renders(scene, tmp_path):
    g, s, imgs, plan, cfg, _ = scene
    with open(tmp_path / "l.tif", "wb") as fl, open(tmp_path / "c.tif", "w+b") as fc:
        with pytest.raises(capi.OchipError, match='layers_geotiff: with "solve" the second sweep reads the file back'):
            host.ortho_mosaic(plan, g, [s], imgs, config=cfg, color_balance="solve", layers_geotiff=fl, cameras_geotiff=fc)
        assert fl.tell() == 0 and fc.tell() == 0  # nothing was written
    moved = io.BytesIO(b"xx")
    moved.seek(2)
    with pytest.raises(capi.OchipError, match='cameras_geotiff: with "solve" the second sweep reads the file back'):
        host.ortho_mosaic(plan, g, [s], imgs, config=cfg, color_balance="solve", layers_geotiff=io.BytesIO(), cameras_geotiff=moved)
    # a single sweep reads nothing back and takes a write-only object
    with open(tmp_path / "l.tif", "wb") as fl, open(tmp_path / "c.tif", "wb") as fc:
        host.ortho_mosaic(plan, g, [s], imgs, config=cfg, layers_geotiff=fl, cameras_geotiff=fc)
    back = host.read_layer_files(tmp_path / "l.tif", tmp_path / "c.tif")
    assert back["bgra"].any()

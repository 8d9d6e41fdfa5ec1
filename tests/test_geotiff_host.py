"""The tiled DEFLATE GeoTIFFs on the CPU route (csrc/deflate_rules.hpp, csrc/host/geotiff.cpp, host.GeoTiffWriter; DESIGN.md
section 4.19).  The yardsticks are outside this project: zlib's inflate (zlib.decompress) reads every tile's stream, libtiff
through Pillow reads every file, and zlib's own Z_HUFFMAN_ONLY stream bounds the size.  A small TIFF reader (geotiff_parse.py)
gives the tags and tile arrays.  Nothing loaded into Python runs under a sanitizer: the rules are driven to their buffer bounds
by a stand-alone program (deflate_rules_driver.cpp) built with the system g++."""
import io
import os
import subprocess
import warnings
import zlib

import numpy as np
import pytest

import geotiff_fixtures as F
import geotiff_parse as P
from opencalibration_amd import capi, host

Image = pytest.importorskip("PIL.Image")
HERE = os.path.dirname(os.path.abspath(__file__))


def written(raster, step=None, **kw):
    """the file of a raster fed in bands of `step` rows (None: whole), with its overview levels"""
    kind = host.OVERVIEW_FLOAT32 if raster.dtype == np.float32 else host.OVERVIEW_RGBA8
    h, w = raster.shape[:2]
    levels = kw.pop("levels", None)
    f = io.BytesIO()
    with host.GeoTiffWriter(f, kind, w, h, **kw) as wr:
        for r in range(0, h, step or h):
            wr.feed(r, raster[r:r + (step or h)])
        wr.finish(levels)
    return f.getvalue()


_files = {}


def file_of(name, big=False):
    """(raster, levels, file bytes) of a fixture with geo tags and overviews, sparse=False: computed once"""
    if (name, big) not in _files:
        raster = F.dsm() if name == "dsm" else F.rgba(name)
        levels = host.ortho_overviews(raster)
        _files[name, big] = (raster, levels, written(raster, geo=F.GEO, bigtiff=big, sparse=False, levels=levels))
    return _files[name, big]


def same_pixels(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(P.as_u32(a), P.as_u32(b))


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("name", F.RGBA + ("dsm",))
def test_every_tile_inflates_and_pillow_reads_the_file(name, big):
    raster, levels, data = file_of(name, big)
    ifds, is_big = P.parse(data)
    assert is_big == big and len(ifds) == 1 + len(levels)
    for ifd, level in zip(ifds, [raster] + levels):
        assert P.check_level(data, ifd, level) == []
    im = Image.open(io.BytesIO(data))
    assert getattr(im, "n_frames", 1) == len(ifds)
    for k, level in enumerate([raster] + levels):
        im.seek(k)
        assert same_pixels(np.asarray(im), level), k


@pytest.mark.parametrize("name", ["half_zero", "dsm"])
def test_tags(name):
    raster, levels, data = file_of(name)
    ifds, _ = P.parse(data)
    rgba = name != "dsm"
    h, w = raster.shape[:2]
    t = ifds[0]
    assert t[256] == (w,) and t[257] == (h,) and t[258] == ((8, 8, 8, 8) if rgba else (32,)) and t[259] == (8,)
    assert t[262] == ((2,) if rgba else (1,)) and t[277] == ((4,) if rgba else (1,)) and t[284] == (1,) and t[317] == (2,)
    assert t[322] == (512,) and t[323] == (512,) and len(t[324]) == len(t[325]) == 6
    assert t[339] == ((1, 1, 1, 1) if rgba else (3,))
    assert (t.get(338) == (2,)) if rgba else (338 not in t)
    assert (t.get(42113) == b"nan\0") if not rgba else (42113 not in t)
    assert t[33550] == (F.GEO["gsd"], F.GEO["gsd"], 0.0) and t[33922] == (0.0, 0.0, 0.0, F.GEO["min_x"], F.GEO["max_y"], 0.0)
    assert t[34735] == (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, F.GEO["epsg"])
    assert 254 not in t
    for k, (o, level) in enumerate(zip(ifds[1:], levels)):
        assert o[254] == (1,) and o[256] == (level.shape[1],) and o[257] == (level.shape[0],) and o[322] == (512,), k
        assert 33550 not in o
    # every level's data lies before its arrays and its IFD; the first tile starts right behind the header
    assert min(o for o in t[324] if o) == 8
    tv = Image.open(io.BytesIO(data)).tag_v2
    assert tv[259] == 8 and tv[317] == 2 and tv[322] == 512 and tv[323] == 512 and tuple(tv[33550]) == t[33550]
    assert tuple(tv[33922]) == t[33922] and tuple(tv[34735]) == t[34735]
    if not rgba:
        assert tv[42113] == "nan"
    # without an EPSG code only the raster type key
    g = dict(F.GEO)
    del g["epsg"]
    assert P.parse(written(raster, geo=g))[0][0][34735] == (1, 1, 0, 1, 1025, 0, 1, 1)
    assert 33550 not in P.parse(written(raster))[0][0]


@pytest.mark.parametrize("name", ["half_zero", "dsm"])
def test_the_same_bytes_however_the_raster_is_fed(name):
    raster, levels, data = file_of(name)
    for step in (512, 100):
        assert written(raster, step, geo=F.GEO, bigtiff=False, sparse=False, levels=levels) == data, step
    f = io.BytesIO()
    host.save_geotiff(f, raster, geo=F.GEO, sparse=False)
    assert f.getvalue() == data


def test_sparse_leaves_out_exactly_the_all_zero_rgba_tiles(tmp_path):
    raster = F.rgba("half_zero")
    data = written(raster)  # sparse is the default
    ifd = P.parse(data)[0][0]
    zero = [(ty, tx) for ty, tx, px in P.padded_tiles(raster) if not px.any()]
    assert zero == [(0, 2), (1, 2)]
    assert P.check_level(data, ifd, raster, sparse_zero_ok=True) == zero
    assert P.check_level(written(F.rgba("zeros")), P.parse(written(F.rgba("zeros")))[0][0], F.rgba("zeros"), True) == \
        [(ty, tx) for ty in range(2) for tx in range(3)]
    d = F.dsm().copy()
    d[:512, :512] = 0.0  # a DSM tile of zeros is written: a reader fills a missing tile with 0.0, never with NaN
    ifd = P.parse(written(d))[0][0]
    assert all(o and c for o, c in zip(ifd[324], ifd[325]))
    path = tmp_path / "dsm.tif"
    host.save_geotiff(path, d, overviews=False)  # a path: opened and closed by the writer
    assert path.read_bytes() == written(d)


def tile_payloads(raster):
    return np.stack([P.predict(px, raster.dtype == np.float32) for _, _, px in P.padded_tiles(raster)])


def huffman_only(payload):
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
    return len(c.compress(payload.tobytes()) + c.flush())


@pytest.mark.parametrize("name", F.COMPRESSIBLE)
def test_no_larger_than_zlib_huffman_only(name):
    """At most 1.05 x zlib's own Huffman-only stream of the same payloads: the 5 % covers the fixed block cutting and the
    heuristic limiter (measured, the ratio to Huffman-only and to zlib level 6: zeros 0.015 / 1.94, constant 0.020 / 1.34,
    ramp 0.61 / 18.0, half_zero 0.36 / 15.6, photo 0.69 / 2.49)."""
    payloads = tile_payloads(F.rgba(name))
    streams = host.deflate_tiles(payloads)
    for s, p in zip(streams, payloads):
        assert zlib.decompress(s) == p.tobytes()
    ours, theirs = sum(map(len, streams)), sum(map(huffman_only, payloads))
    print(name, ours, theirs, ours / theirs, sum(len(zlib.compress(p.tobytes(), 6)) for p in payloads))
    assert ours <= 1.05 * theirs


def test_noise_is_stored_and_zeros_are_chains_of_matches():
    noise, = host.deflate_tiles(tile_payloads(F.rgba("noise")))
    assert len(noise) == P.MAX_STREAM == 1048667 and noise[:3] == b"\x78\x9c\x00" and noise[3:7] == b"\xff\xff\x00\x00"
    # a block of zeros is 4 literals and 64 matches: 64 x 13 bits in the fixed code, which a dynamic code of one-bit lengths
    # and distances undercuts even with its header - the smaller of the two is taken, 31 bytes a block
    zeros, = host.deflate_tiles(np.zeros((1, P.PAYLOAD), np.uint8))
    assert zeros[:2] == b"\x78\x9c" and zeros[2] & 7 == 4  # BFINAL 0, BTYPE 10
    assert len(zeros) < 64 * 13 * 64 // 8
    # a literal-only block over all 256 values, zeros behind it
    flat = np.zeros((1, P.PAYLOAD), np.uint8)
    flat[0, :F.SEGMENT] = F.quiet(F.SEGMENT) | np.tile(np.repeat(np.arange(4, dtype=np.uint8) << 6, 4), F.SEGMENT // 16)
    s, = host.deflate_tiles(flat)
    assert zlib.decompress(s) == flat.tobytes()


def test_crafted_payloads():
    names, payloads = F.crafted()
    streams = host.deflate_tiles(payloads)
    for name, s, p in zip(names, streams, payloads):
        assert len(s) <= P.MAX_STREAM and zlib.decompress(s) == p.tobytes(), name
    # each alone gives the same stream: nothing is read from the payload before
    for k in (names.index("first_row"), names.index("fibonacci")):
        assert host.deflate_tiles(payloads[k:k + 1]) == streams[k:k + 1]
    # the first block of the Fibonacci payload is dynamic and its literal code reaches 15 bits
    fib = streams[names.index("fibonacci")]
    assert fib[2] & 7 == 4  # BFINAL 0, BTYPE 10


def kraft(lens, limit):
    return sum(1 << (limit - int(v)) for v in lens if v)


def test_code_lengths():
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    cases = [(fib, 15), (fib[:19], 7), ([5] * 286, 15), ([5] * 286, 9), ([0, 0, 3, 0], 15), ([0, 4, 3, 0], 15), ([0] * 4, 15),
             (list(np.random.default_rng(3).integers(0, 1000, 286)), 15), (list(np.random.default_rng(4).integers(0, 3, 30)), 15)]
    for counts, limit in cases:
        lens = host.deflate_code_lengths(counts, limit)
        used = [i for i, c in enumerate(counts) if c]
        assert all((c == 0) == (v == 0) for c, v in zip(counts, lens)) and max(lens, default=0) <= limit
        assert kraft(lens, limit) <= 1 << limit
        if len(used) >= 2:
            assert kraft(lens, limit) == 1 << limit
        for a in used:  # a more frequent symbol never gets a longer code
            for b in used:
                assert not (counts[a] > counts[b] and lens[a] > lens[b])
    assert max(host.deflate_code_lengths(fib, 15)) == 15 and list(host.deflate_code_lengths([0, 0, 3, 0], 15)) == [0, 0, 1, 0]
    assert list(host.deflate_code_lengths([7, 7, 7, 7], 15)) == [2, 2, 2, 2]
    with pytest.raises(capi.OchipError):
        host.deflate_code_lengths([1] * 20, 4)


class NoSeek(io.BytesIO):
    def seekable(self):
        return False


def test_refusals():
    raster = F.rgba("ramp")
    h, w = raster.shape[:2]
    with pytest.raises(capi.OchipError, match="seekable"):
        host.GeoTiffWriter(NoSeek(), host.OVERVIEW_RGBA8, w, h)
    with pytest.raises(capi.OchipError):
        host.GeoTiffWriter(io.BytesIO(), 2, w, h)
    with pytest.raises(capi.OchipError, match="0 x 4"):
        host.GeoTiffWriter(io.BytesIO(), host.OVERVIEW_RGBA8, 0, 4)
    with host.GeoTiffWriter(io.BytesIO(), host.OVERVIEW_RGBA8, w, h) as wr:
        with pytest.raises(capi.OchipError, match=r"rows 8 \.\. 16 where row 0 is next \(a gap\)"):
            wr.feed(8, raster[8:16])
        wr.feed(0, raster[:20])
        with pytest.raises(capi.OchipError, match=r"rows 16 \.\. 24 where row 20 is next \(an overlap\)"):
            wr.feed(16, raster[16:24])
        with pytest.raises(capi.OchipError, match="rows from 20"):
            wr.feed(20, raster[20:30, :100])  # a wrong width
        with pytest.raises(capi.OchipError, match="rows from 20"):
            wr.feed(20, np.zeros((4, w), np.float32))  # a wrong kind
        with pytest.raises(capi.OchipError, match=r"beyond the raster's 511"):
            wr.feed(20, np.concatenate([raster[20:], raster[:40]]))
        with pytest.raises(capi.OchipError, match=r"rows 20 \.\. 511 were never fed"):
            wr.finish()
    f = io.BytesIO()
    wr = host.GeoTiffWriter(f, host.OVERVIEW_RGBA8, w, h)
    wr.feed(0, raster)
    with pytest.raises(capi.OchipError, match="overview levels"):
        wr.finish([raster])
    wr.close()
    f = io.BytesIO()
    wr = host.GeoTiffWriter(f, host.OVERVIEW_RGBA8, w, h)
    wr.feed(0, raster)
    wr.finish()
    with pytest.raises(capi.OchipError):
        wr.feed(511, raster[:1])
    with pytest.raises(capi.OchipError):
        wr.finish()
    assert same_pixels(np.asarray(Image.open(io.BytesIO(f.getvalue()))), raster)
    L = host.load()
    enc = host._TileEncoder(host.OVERVIEW_RGBA8, 4, 4, None, True)
    dead = enc.h
    enc.feed(0, 4, np.zeros((4, 4, 4), np.uint8).ctypes.data, False)
    enc.finish()
    with pytest.raises(capi.OchipError, match="after finish"):
        enc.feed(4, 1, np.zeros((1, 4, 4), np.uint8).ctypes.data, False)
    enc.close()
    assert L.och_geotiff_finish(dead) == -1 and "not a live" in L.och_geotiff_last_error().decode()


def test_mosaic_writes_both_files():
    """ortho_mosaic(geotiff=, dsm_geotiff=) on the CPU route: the files decode to the returned mosaic, to the DSM and to the
    levels overviews=True returns; without the arguments the pixels are the same."""
    from layers_fixtures import four_camera_scene
    from tile_progress_fixtures import mosaic_plan

    g, s, imgs = four_camera_scene(seed=4)
    plan = mosaic_plan(0.05)
    cfg = dict(tile_size=160, blend_transition_radius=10)
    plain = host.ortho_mosaic(plan, g, [s], imgs, config=cfg, tile_rows=1)
    f, fd = io.BytesIO(), io.BytesIO()
    out, over = host.ortho_mosaic(plan, g, [s], imgs, config=cfg, tile_rows=1, overviews=True, geotiff=f, dsm_geotiff=fd,
                                  geo=dict(epsg=32632))
    assert np.array_equal(out, plain)
    assert np.array_equal(host.ortho_mosaic(plan, g, [s], imgs, config=cfg, tile_rows=1, geotiff=io.BytesIO()), plain)
    dsm = host.dsm_render(plan, [s])
    dsm = dsm[0] if isinstance(dsm, tuple) else dsm
    for data, raster, levels in ((f.getvalue(), out, over["rgba"]), (fd.getvalue(), dsm, over["dsm"])):
        ifds, _ = P.parse(data)
        assert len(ifds) == 1 + len(levels)
        im = Image.open(io.BytesIO(data))
        for k, level in enumerate([raster] + list(levels)):
            P.check_level(data, ifds[k], level, sparse_zero_ok=True)
            im.seek(k)
            assert same_pixels(np.asarray(im), level), k
        assert ifds[0][33922] == (0.0, 0.0, 0.0, plan["min_x"], plan["max_y"], 0.0) and ifds[0][33550][0] == plan["gsd"]
        assert ifds[0][34735][-1] == 32632


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("deflate_rules") / "driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-o", exe, os.path.join(HERE, "deflate_rules_driver.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        warnings.warn("the sanitizer runtimes do not link here: the driver runs plain")
        subprocess.run(cmd, check=True)
    return exe


def test_rules_under_sanitizers(driver):
    r = subprocess.run([driver], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-3000:]
    assert "noise: 1048667 bytes" in r.stdout

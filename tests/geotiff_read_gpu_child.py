"""The scenarios of test_gpu_geotiff_read.py, run in a child process that brings torch up before libochip.so (as
geotiff_gpu_child.py does) and holds one capi.Context(0).  `python geotiff_read_gpu_child.py <tests dir> <repo dir>` runs every
scenario and prints one JSON line {scenario: "ok" or the failure's traceback}.  A scenario that ends in a device error ends the
run: the ones after it are reported as not run.  The yardstick is the host route of the same library (ctx None), which
test_geotiff_read_host.py holds against zlib and the arrays the files were built from.  Only well-formed streams reach a
kernel: the damaged ones run through the same rules on the host, under the sanitizers."""
import io
import json
import os
import sys
import tempfile
import traceback
import zlib

import numpy as np
import torch

torch.cuda.init()
if __name__ == "__main__":
    sys.path[:0] = sys.argv[1:3]

import geotiff_fixtures as G  # noqa: E402
import geotiff_read_fixtures as R  # noqa: E402
import mesh_points_fixtures as M  # noqa: E402
from layers_fixtures import four_camera_scene  # noqa: E402
from tile_progress_fixtures import mosaic_plan  # noqa: E402
from opencalibration_amd import host  # noqa: E402

MOSAIC = (0.05, 160, 1)  # gsd, tile_size, tile_rows: the scene of geotiff_gpu_child.py


def both_routes(ctx, streams, expects, what, budget=0):
    want = host.inflate_report(streams, expects)
    got = host.inflate_report(streams, expects, ctx=ctx, budget=budget)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{what}: stream {i}: status and bytes {g[:2]} against the host route's {w[:2]}"
    return got


def scenario_zoo_batch(ctx):
    zoo = R.zoo()
    got = both_routes(ctx, [z for _, z, _ in zoo], [len(d) for _, _, d in zoo], "the zoo in one batch")
    for (name, _, data), (status, produced, payload) in zip(zoo, got):
        assert status == host.INFLATE_OK and payload == data, name


def scenario_zoo_one_by_one(ctx):
    for name, z, data in R.zoo():
        got = host.inflate_report([z], [len(data)], ctx=ctx)
        assert got == [(host.INFLATE_OK, len(data), data)], name


def scenario_chunk_and_ring_sizes(ctx):
    streams, datas = [], []
    for n in (R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 2 * R.CHUNK, R.RING - 1, R.RING, R.RING + 1, 3 * R.RING + R.CHUNK):
        for kind in R.KINDS:
            data = R.payload(kind, n)
            for kw in (dict(level=6), dict(level=0), dict(strategy=zlib.Z_FIXED), dict(flush=zlib.Z_FULL_FLUSH)):
                streams.append(R.deflate(data, **kw)), datas.append(data)
    got = both_routes(ctx, streams, [len(d) for d in datas], "sizes around the chunk and the ring")
    for k, ((status, _, payload), data) in enumerate(zip(got, datas)):
        assert status == host.INFLATE_OK and payload == data, k


def scenario_hand_cases(ctx):
    cases = R.hand_cases()
    got = both_routes(ctx, [z for z, _ in cases.values()], [len(d) for _, d in cases.values()], "the hand-assembled cases")
    for name, (status, _, payload) in zip(cases, got):
        assert status == host.INFLATE_OK and payload == cases[name][1], name
    for name, (z, data) in cases.items():
        assert host.inflate_streams([z], len(data), ctx=ctx) == [data], name


def scenario_own_streams(ctx):
    names, payloads = G.crafted()
    payloads = np.concatenate([payloads, np.random.default_rng(3).integers(0, 256, (1, G.PAYLOAD), dtype=np.uint8)])
    streams = host.deflate_tiles(payloads, ctx=ctx)
    assert len(streams[-1]) == host.GEOTIFF_MAX_STREAM                     # the stored 17-block fallback
    got = host.inflate_streams(streams, G.PAYLOAD, ctx=ctx)
    for k, g in enumerate(got):
        assert g == payloads[k].tobytes(), k


def scenario_not_ok_among_ok(ctx):
    """well-formed streams that are not OK, each between accepted ones whose payloads stay intact"""
    data = R.payload("text", 40000)
    good = zlib.compress(data, 6)
    left, right = R.payload("ramp", 70001), R.payload("noise", 1023)
    cases = {"wrong_adler": (good[:-1] + bytes([good[-1] ^ 1]), len(data)), "shorter_than_expect": (good, len(data) + 1),
             "longer_than_expect": (good, len(data) - 1), "byte_behind_the_checksum": (good + b"\0", len(data)),
             "much_longer_than_expect": (zlib.compress(bytes(1 << 20)), 1000)}
    streams, expects = [], []
    for z, e in cases.values():
        streams += [zlib.compress(left, 1), z, zlib.compress(right, 9)]
        expects += [len(left), e, len(right)]
    got = both_routes(ctx, streams, expects, "streams that are not OK among accepted ones")
    for k, name in enumerate(cases):
        assert got[3 * k] == (host.INFLATE_OK, len(left), left) and got[3 * k + 2] == (host.INFLATE_OK, len(right), right), name
        assert got[3 * k + 1][0] == host.INFLATE_CORRUPT and got[3 * k + 1][2] is None, name
    try:
        host.inflate_streams(streams[:3], expects[:3], ctx=ctx)
    except host.GeoTiffError as e:
        assert e.status == "corrupt" and "stream 1 of 3" in str(e)
    else:
        raise AssertionError("a wrong Adler-32 was not refused")


def read_both(ctx, data, what, windows=None, budget=0):
    """every level and window of the file through the host route, the device route to numpy and the device route to a tensor"""
    with host.GeoTiffReader(data) as hr, host.GeoTiffReader(data, ctx=ctx, budget=budget) as dr:
        assert (dr.width, dr.height, dr.samples, dr.levels, dr.geo) == (hr.width, hr.height, hr.samples, hr.levels, hr.geo)
        for level in range(len(hr.levels) + 1):
            h = hr.height if level == 0 else hr.levels[level - 1][0]
            for row0, rows in (windows if windows and level == 0 else [(0, h)]):
                want = hr.read(row0, rows, level=level)
                got = dr.read(row0, rows, level=level)
                assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), \
                    f"{what}: level {level} rows {row0} + {rows} through numpy"
                t = dr.read(row0, rows, level=level, on_device=True)
                assert t.is_cuda and tuple(t.shape) == want.shape and t.cpu().numpy().tobytes() == want.tobytes(), \
                    f"{what}: level {level} rows {row0} + {rows} on the device"
        return dr.launches()


def scenario_reader_written_files(ctx):
    for name in G.RGBA + ("dsm",):
        a = G.dsm() if name == "dsm" else G.rgba(name)
        for kw in (dict(bigtiff=False, sparse=True), dict(bigtiff=True, sparse=False)):
            f = io.BytesIO()
            host.save_geotiff(f, a, geo=G.GEO, **kw)
            read_both(ctx, f.getvalue(), f"{name} {kw}")
            with host.GeoTiffReader(f.getvalue(), ctx=ctx) as rd:
                assert rd.read().tobytes() == a.tobytes(), name


def scenario_reader_matrix(ctx):
    sizes = ((1, 1), (17, 33), (512, 512), (513, 511), (1100, 700))
    k = 0
    for layout in (1, 3, 4, "f"):
        for predictor in (1, 2):
            for tile in (16, 48, 512):
                for w, h in sizes:
                    k += 1
                    a = R.raster(layout, h, w)
                    if k % 3 == 0 and layout != "f":
                        a = a.copy()
                        a[:, : w // 2] = 0
                    data = R.build_tiff(a, tile=(tile, tile), big=k % 2 == 1, predictor=predictor, compression=(8, 32946)[k // 2 % 2],
                                        level=(6, 1, 9, 0)[k % 4], sparse=k % 3 == 0)
                    windows = [(0, h), (h - 1, 1)]
                    if h > tile:
                        windows += [(tile - 1, 2), ((h - 1) // tile * tile, h - (h - 1) // tile * tile)]
                    if h > 3:
                        windows.append((1, 2))
                    read_both(ctx, data, f"layout {layout} predictor {predictor} tile {tile} raster {w} x {h}", windows)
                    with host.GeoTiffReader(data, ctx=ctx) as rd:
                        out = torch.zeros((h, w) if layout == "f" else (h, w, layout), dtype=torch.float32 if layout == "f" else torch.uint8,
                                          device="cuda:0")
                        assert rd.read(out=out, on_device=True) is out and out.cpu().numpy().tobytes() == a.tobytes()


def scenario_two_readers(ctx):
    a, b = R.raster(4, 100, 150), R.raster("f", 90, 70)
    da, db = R.build_tiff([a, a[::2, ::2].copy()], tile=(64, 32)), R.build_tiff(b, tile=(16, 16))
    with host.GeoTiffReader(da, ctx=ctx) as ra, host.GeoTiffReader(db, ctx=ctx) as rb:
        ta = ra.read(0, 40, on_device=True)
        tb = rb.read(10, 70, on_device=True)
        ta2 = ra.read(40, 60, on_device=True)
        l1 = ra.read(level=1)
        assert torch.cat([ta, ta2]).cpu().numpy().tobytes() == a.tobytes() and tb.cpu().numpy().tobytes() == b[10:80].tobytes()
        assert l1.tobytes() == a[::2, ::2].tobytes()


def scenario_scratch_budget(ctx):
    """a request larger than one launch's scratch budget: 16 x 16 tiles and a budget of a few of them"""
    a = R.raster(4, 100, 200)
    data = R.build_tiff(a, tile=(16, 16), level=0)                        # 13 x 7 stored tiles of 1 024 + 11 bytes
    launches = read_both(ctx, data, "a budget of 10 000 bytes", budget=10000)
    assert launches == 2 * 23, launches                                  # 91 tiles, 4 a launch, two full reads
    assert read_both(ctx, data, "the default budget") == 2
    streams = [zlib.compress(R.payload("ramp", 5000 + 37 * i)) for i in range(40)]
    got = both_routes(ctx, streams, [5000 + 37 * i for i in range(40)], "an inflate over many launches", budget=20000)
    assert all(g[0] == host.INFLATE_OK for g in got)
    big = R.payload("text", 300000)
    assert host.inflate_streams([zlib.compress(big)], len(big), ctx=ctx, budget=1000) == [big]   # a launch takes at least one stream


def scenario_mosaic(ctx):
    """the writer's device route read back by the reader's device route without a host pixel"""
    gsd, t, tile_rows = MOSAIC
    g, s, imgs = four_camera_scene(seed=4)
    plan = mosaic_plan(gsd)
    cfg = dict(tile_size=t, blend_transition_radius=10)
    dimg = [torch.from_numpy(im).to("cuda:0") for im in imgs]
    with host.OrthoMesh(ctx, [s]) as mesh:
        f, fd = io.BytesIO(), io.BytesIO()
        out, over = host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, tile_rows=tile_rows, overviews=True, geotiff=f, dsm_geotiff=fd)
        dsm = host.dsm_render(plan, [s], mesh=mesh)
        if not isinstance(dsm, torch.Tensor):
            dsm = torch.from_numpy(np.ascontiguousarray(dsm)).to("cuda:0")
        ctx.synchronize()
        torch.cuda.synchronize()
    for data, raster, levels in ((f.getvalue(), out, over["rgba"]), (fd.getvalue(), dsm, over["dsm"])):
        for k, want in enumerate([raster] + list(levels)):
            got, geo = host.load_geotiff(data, ctx=ctx, level=k, on_device=True)
            assert got.is_cuda and got.shape == want.shape and got.dtype == want.dtype
            same = torch.equal(got, want) if got.dtype == torch.uint8 else torch.equal(got.view(torch.int32), want.view(torch.int32))
            assert same, f"level {k}"
            assert (geo["min_x"], geo["max_y"], geo["gsd_x"], geo["gsd_y"]) == (plan["min_x"], plan["max_y"], plan["gsd"], plan["gsd"])


def scenario_textured_obj(ctx):
    surfaces = [M.mesh("minimal")]
    plan = dict(width=64, height=48, gsd=0.0371, min_x=-12.5, max_x=-10.1256, min_y=81.4692, max_y=83.25, mean_camera_z=50.0)
    rgba = np.random.default_rng(0).integers(0, 256, (48, 64, 4), dtype=np.uint8)
    d = tempfile.mkdtemp(prefix="geotiff_read_obj_")
    tif = os.path.join(d, "orthomosaic.tif")
    host.save_geotiff(tif, rgba, geo=dict(min_x=plan["min_x"], max_y=plan["max_y"], gsd=plan["gsd"], epsg=32632))
    os.mkdir(os.path.join(d, "a")), os.mkdir(os.path.join(d, "b"))
    one = host.save_textured_obj(os.path.join(d, "a", "site.obj"), surfaces, rgba, plan, jpeg=True)
    two = host.save_textured_obj_from_geotiff(os.path.join(d, "b", "site.obj"), surfaces, tif, jpeg=True, ctx=ctx)
    assert one == two
    for ext in ("obj", "mtl", "jpg"):
        assert open(os.path.join(d, "a", "site." + ext), "rb").read() == open(os.path.join(d, "b", "site." + ext), "rb").read(), ext


def scenario_refusals(ctx):
    """arguments that are refused before anything is launched"""
    L = host.load()
    rd = host._TileReader(4, False, 100, 100, 16, 16, 2, ctx)
    one = np.zeros(8, np.uint64)
    bad = np.zeros(1, np.int64)
    calls = {
        "65535 streams": lambda: L.och_geotiff_reader_inflate(rd.h, 65536, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data, 8,
                                                              one.ctypes.data, one.ctypes.data),
        "offsets are NULL": lambda: L.och_geotiff_reader_inflate(rd.h, 1, one.ctypes.data, None, None, None, 0, None, None),
        "expect, status or bytes is NULL": lambda: L.och_geotiff_reader_inflate(rd.h, 1, one.ctypes.data, one.ctypes.data, None, None, 0, None, None),
        "not inside the raster": lambda: L.och_geotiff_reader_read(rd.h, 7, one.ctypes.data, one.ctypes.data, 90, 11, one.ctypes.data, 0,
                                                                   bad.ctypes.data_as(host.C.POINTER(host.C.c_int64))),
        "not those of the tile rows": lambda: L.och_geotiff_reader_read(rd.h, 6, one.ctypes.data, one.ctypes.data, 0, 10, one.ctypes.data, 0,
                                                                        bad.ctypes.data_as(host.C.POINTER(host.C.c_int64))),
    }
    for text, call in calls.items():
        assert call() == -1 and text in rd._error(), (text, rd._error())
    assert rd.launches() == 0
    dead = rd.h
    rd.close()
    assert L.och_geotiff_reader_inflate(dead, 0, None, None, None, None, 0, None, None) == -1
    assert "not a live" in L.och_geotiff_read_last_error().decode()
    try:
        host._TileReader(2, False, 100, 100, 16, 16, 2, ctx)
    except host.GeoTiffError as e:
        assert e.status == "refused" and "1, 3 or 4" in str(e)
    else:
        raise AssertionError("two samples were not refused")


SCENARIOS = dict(zoo_batch=scenario_zoo_batch, zoo_one_by_one=scenario_zoo_one_by_one, chunk_and_ring_sizes=scenario_chunk_and_ring_sizes,
                 hand_cases=scenario_hand_cases, own_streams=scenario_own_streams, not_ok_among_ok=scenario_not_ok_among_ok,
                 reader_written_files=scenario_reader_written_files, reader_matrix=scenario_reader_matrix, two_readers=scenario_two_readers,
                 scratch_budget=scenario_scratch_budget, mosaic=scenario_mosaic, textured_obj=scenario_textured_obj, refusals=scenario_refusals)


if __name__ == "__main__":
    from opencalibration_amd import capi

    only = sys.argv[3].split(",") if len(sys.argv) > 3 else None
    ctx = capi.Context(0)
    res, device_error = {}, False
    for name, fn in SCENARIOS.items():
        if only and name not in only:
            continue
        try:
            fn(ctx)
            res[name] = "ok"
        except AssertionError:
            res[name] = traceback.format_exc()
        except Exception:  # a device error: nothing more runs on that device
            res[name] = traceback.format_exc()
            device_error = True
            break
    for name in SCENARIOS:
        if not only or name in only:
            res.setdefault(name, "not run: an earlier scenario ended in an error")
    print(json.dumps(res), flush=True)
    if not device_error:
        ctx.close()

"""The scenarios of test_gpu_geotiff.py, run in a child process that brings torch up before libochip.so (as jpeg_gpu_child.py
does) and holds one capi.Context(0).  `python geotiff_gpu_child.py <tests dir> <repo dir>` runs every scenario and prints one
JSON line {scenario: "ok" or the failure's traceback}.  A scenario that ends in a device error ends the run: the ones after it
are reported as not run.  The yardstick is the CPU route of the same library (ctx None), which test_geotiff_host.py holds
against zlib's inflate and libtiff."""
import io
import json
import sys
import traceback

import numpy as np
import torch

torch.cuda.init()
if __name__ == "__main__":
    sys.path[:0] = sys.argv[1:3]

import geotiff_fixtures as F  # noqa: E402
import geotiff_parse as P  # noqa: E402
from layers_fixtures import four_camera_scene  # noqa: E402
from tile_progress_fixtures import mosaic_plan  # noqa: E402
from opencalibration_amd import capi, host  # noqa: E402

MOSAIC = (0.05, 160, 1)  # gsd, tile_size, tile_rows: the smallest scene of the mosaic GPU tests, 210 x 180


def to_device(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()  # the kernels run on the context's own stream
    return t


def same(got, want, what):
    if got != want:
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"{what}: {len(got)} bytes against {len(want)}, first difference at byte {at}")


def written(raster, levels, step, ctx, on_device, big, sparse, geo=F.GEO):
    kind = host.OVERVIEW_FLOAT32 if str(raster.dtype).endswith("float32") else host.OVERVIEW_RGBA8
    h, w = int(raster.shape[0]), int(raster.shape[1])
    f = io.BytesIO()
    with host.GeoTiffWriter(f, kind, w, h, geo=geo, ctx=ctx, on_device=on_device, bigtiff=big, sparse=sparse) as wr:
        for r in range(0, h, step):
            wr.feed(r, raster[r:r + step])
        wr.finish(levels)
    return f.getvalue()


def scenario_raster(ctx, name):
    raster = F.dsm() if name == "dsm" else F.rgba(name)
    levels = host.ortho_overviews(raster)
    d_raster, d_levels = to_device(raster), [to_device(l) for l in levels]
    for big in (False, True):
        for sparse in (True, False):
            want = written(raster, levels, raster.shape[0], None, False, big, sparse)
            for step in (512, 100):
                same(written(d_raster, d_levels, step, ctx, True, big, sparse), want,
                     f"{name} bigtiff={big} sparse={sparse}: device tensors in bands of {step}")
            same(written(raster, levels, raster.shape[0], ctx, False, big, sparse), want,
                 f"{name} bigtiff={big} sparse={sparse}: numpy through the device")
    f = io.BytesIO()
    host.save_geotiff(f, d_raster, geo=F.GEO, ctx=ctx, bigtiff=False, sparse=True)
    same(f.getvalue(), written(raster, levels, raster.shape[0], None, False, False, True), f"{name}: save_geotiff of a device tensor")


def scenario_crafted(ctx):
    names, payloads = F.crafted()
    want = host.deflate_tiles(payloads)
    got = host.deflate_tiles(payloads, ctx=ctx)
    assert len(got) == len(want)
    for name, g, w in zip(names, got, want):
        same(g, w, name)
    k = names.index("first_row")
    same(host.deflate_tiles(payloads[k:k + 1], ctx=ctx)[0], want[k], "first_row alone")


def refused(text, call, *args, **kwargs):
    try:
        call(*args, **kwargs)
    except capi.OchipError as e:
        assert text in str(e), str(e)
        return
    raise AssertionError("not refused: " + text)


def scenario_refusals(ctx):
    raster = to_device(F.rgba("ramp"))
    h, w = raster.shape[:2]
    refused("0 x 4", host.GeoTiffWriter, io.BytesIO(), host.OVERVIEW_RGBA8, 0, 4, ctx=ctx, on_device=True)
    f = io.BytesIO()
    with host.GeoTiffWriter(f, host.OVERVIEW_RGBA8, w, h, geo=F.GEO, ctx=ctx, on_device=True) as wr:
        refused("rows 8 .. 16 where row 0 is next (a gap)", wr.feed, 8, raster[8:16])
        wr.feed(0, raster[:20])
        refused("rows 16 .. 24 where row 20 is next (an overlap)", wr.feed, 16, raster[16:24])
        refused("beyond the raster's 511", wr.feed, 20, torch.cat([raster[20:], raster[:40]]))
        refused("rows 20 .. 511 were never fed", wr.finish)
        wr.feed(20, raster[20:])
        wr.finish()
    same(f.getvalue(), written(F.rgba("ramp"), None, 511, None, False, None, True), "the writer after its refusals")
    L = host.load()
    enc = host._TileEncoder(host.OVERVIEW_RGBA8, 4, 4, ctx, True)
    dead = enc.h
    enc.close()
    assert L.och_geotiff_finish(dead) == -1 and "not a live" in L.och_geotiff_last_error().decode()


def scenario_mosaic(ctx):
    gsd, t, tile_rows = MOSAIC
    g, s, imgs = four_camera_scene(seed=4)
    plan = mosaic_plan(gsd)
    cfg = dict(tile_size=t, blend_transition_radius=10)
    dimg = [torch.from_numpy(im).to("cuda:0") for im in imgs]
    with host.OrthoMesh(ctx, [s]) as mesh:
        plain = host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, tile_rows=tile_rows)
        f, fd = io.BytesIO(), io.BytesIO()
        out, over = host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, tile_rows=tile_rows, overviews=True, geotiff=f,
                                      dsm_geotiff=fd)
        assert isinstance(out, torch.Tensor) and torch.equal(out, plain)  # the raster unchanged
        only = host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, tile_rows=tile_rows, geotiff=io.BytesIO())
        assert isinstance(only, torch.Tensor) and torch.equal(only, plain)
        dsm = host.dsm_render(plan, [s], mesh=mesh)
        if not isinstance(dsm, torch.Tensor):
            dsm = to_device(dsm)
        ctx.synchronize()
        torch.cuda.synchronize()
        from PIL import Image

        for data, raster, levels in ((f.getvalue(), out, over["rgba"]), (fd.getvalue(), dsm, over["dsm"])):
            rasters = [raster.cpu().numpy()] + [l.cpu().numpy() for l in levels]
            ifds, _ = P.parse(data)
            assert len(ifds) == len(rasters)
            im = Image.open(io.BytesIO(data))
            for k, level in enumerate(rasters):
                P.check_level(data, ifds[k], level, sparse_zero_ok=True)
                im.seek(k)
                assert np.array_equal(P.as_u32(np.asarray(im)), P.as_u32(level)), k
            same(data, written(rasters[0], rasters[1:], rasters[0].shape[0], None, False, None, True,
                               {k: plan[k] for k in ("min_x", "max_y", "gsd")}), "the mosaic's file, CPU route")


def scenarios():
    s = {f"raster_{name}": (scenario_raster, name) for name in F.RGBA + ("dsm",)}
    s.update(crafted=(scenario_crafted,), refusals=(scenario_refusals,), mosaic=(scenario_mosaic,))
    return s


if __name__ == "__main__":
    ctx = capi.Context(0)
    res, device_error = {}, False
    for name, (fn, *args) in scenarios().items():
        try:
            fn(ctx, *args)
            res[name] = "ok"
        except AssertionError:
            res[name] = traceback.format_exc()
        except Exception:  # a device error: nothing more runs on that device
            res[name] = traceback.format_exc()
            device_error = True
            break
    for name in scenarios():
        res.setdefault(name, "not run: an earlier scenario ended in an error")
    print(json.dumps(res), flush=True)
    if not device_error:
        ctx.close()

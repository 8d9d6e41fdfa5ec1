"""The scenarios of test_gpu_jpeg.py, run in a child process that brings torch up before libochip.so (as
tile_progress_gpu_child.py does) and holds one capi.Context(0).  `python jpeg_gpu_child.py <tests dir> <repo dir>` runs every
scenario and prints one JSON line {scenario: "ok" or the failure's traceback}.  A scenario that ends in a device error ends
the run: the ones after it are reported as not run.  The yardstick is the CPU route of the same library (ctx None), which
test_jpeg_host.py holds against libjpeg-turbo's bytes."""
import io
import json
import sys
import traceback

import numpy as np
import torch

torch.cuda.init()
if __name__ == "__main__":
    sys.path[:0] = sys.argv[1:3]

import jpeg_fixtures as F  # noqa: E402
from layers_fixtures import four_camera_scene  # noqa: E402
from tile_progress_fixtures import mosaic_plan  # noqa: E402
from opencalibration_amd import capi, host  # noqa: E402

# (name, content, height, width, quality): 63, 64 and 65 MCUs in a row - a wavefront's worth less one, exact and one more; 257 x
# 17 MCUs, workgroup runs of 4 that do not divide the row; 16 384 MCUs of noise - megabytes of scan, several blocks of both
# scans, many stuffed bytes, a download guess that falls short; 4 bytes an MCU, many MCUs per stored word; ZRL symbols; and
# 188 x 188 MCUs, more than one pass holds, so the predictors and the partial byte cross a pass inside one feed
LARGE = [("row_of_63_mcus", "noise", 16, 1008, 95), ("row_of_64_mcus", "noise", 16, 1024, 95), ("row_of_65_mcus", "noise", 16, 1040, 95),
         ("ramp_272x4112", "ramp", 272, 4112, 95), ("noise_2048x2048", "noise", 2048, 2048, 95), ("flat_48x64", "flat", 48, 64, 95),
         ("flat_1024x1024", "flat", 1024, 1024, 95), ("checker_32x48_q50", "checker", 32, 48, 50),
         ("checker_256x256_q50", "checker", 256, 256, 50), ("two_passes_3000x3000", "ramp", 3000, 3000, 95)]
SPLITS = (1, 7, 16, 17, 100)
SPLIT_SHAPE = (203, 75)
MOSAIC = (0.05, 160, 1)  # gsd, tile_size, tile_rows: 210 x 180 in bands of 160 and 20 rows

_cpu = {}


def cpu_route(kind, h, w, q=95, seed=0):
    """host.encode_jpeg of a content on the CPU route: computed once, shared, left unchanged"""
    key = (kind, h, w, q, seed)
    if key not in _cpu:
        _cpu[key] = host.encode_jpeg(F.content(kind, h, w, seed), quality=q)
    return _cpu[key]


def to_device(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()  # the kernels run on the context's own stream
    return t


def same(got, want, what):
    if got != want:
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"{what}: {len(got)} bytes against {len(want)}, first difference at byte {at}")


def check(ctx, kind, h, w, q=95, seed=0):
    rgb = F.content(kind, h, w, seed)
    want = cpu_route(kind, h, w, q, seed)
    same(host.encode_jpeg(to_device(F.rgba_of(rgb)), ctx=ctx, quality=q), want, f"{kind} {h}x{w} q{q}: device RGBA tensor")
    return rgb, want


def scenario_shape(ctx, shape):
    h, w = shape
    for kind in F.CONTENTS:
        rgb, want = check(ctx, kind, h, w, seed=h * 131 + w)
        same(host.encode_jpeg(rgb, ctx=ctx), want, f"{kind} {h}x{w}: host RGB array through the device")


def scenario_large(ctx, case):
    _, kind, h, w, q = case
    check(ctx, kind, h, w, q, seed=3)


def fed(ctx, raster, step, on_device):
    h, w = raster.shape[:2]
    out = []
    with host.JpegEncoder(w, h, ctx=ctx, on_device=on_device) as e:
        for r in range(0, h, step):
            e.feed(r, raster[r:r + step])
            out.append(e.collect())
        out.append(e.finish())
    return b"".join(out)


def scenario_splits(ctx):
    """bands of 1, 7, 16, 17 and 100 rows: the carried rows, the predictors and the partial byte survive the band edges"""
    h, w = SPLIT_SHAPE
    rgb = F.noise(h, w, 11)
    want = cpu_route("noise", h, w, 95, 11)
    d_rgba = to_device(F.rgba_of(rgb))
    for step in SPLITS + (h,):
        same(fed(ctx, d_rgba, step, True), want, f"device tensors, bands of {step} rows")
        same(fed(ctx, rgb, step, False), want, f"host arrays, bands of {step} rows")
    # without a collect between the feeds
    with host.JpegEncoder(w, h, ctx=ctx, on_device=True) as e:
        for r in range(0, h, 17):
            e.feed(r, d_rgba[r:r + 17])
        assert e.pending() > 600
        same(e.collect() + e.finish(), want, "device tensors, bands of 17 rows, one collect")


def scenario_two_encoders(ctx):
    a, b = F.noise(70, 90, 21), F.ramp(53, 200)
    da, db = to_device(F.rgba_of(a)), to_device(F.rgba_of(b))
    out_a, out_b = [], []
    with host.JpegEncoder(90, 70, ctx=ctx, on_device=True) as ea, host.JpegEncoder(200, 53, ctx=ctx, quality=50, on_device=True) as eb:
        for r in range(0, 70, 20):
            ea.feed(r, da[r:r + 20])
            if r < 53:
                eb.feed(r, db[r:r + 20])
            out_b.append(eb.collect())
            out_a.append(ea.collect())
        out_a.append(ea.finish())
        out_b.append(eb.finish())
    same(b"".join(out_a), host.encode_jpeg(a), "the first of two encoders")
    same(b"".join(out_b), host.encode_jpeg(b, quality=50), "the second of two encoders")


def scenario_qualities(ctx):
    for q in (1, 50, 100):
        check(ctx, "noise", 33, 47, q, seed=5)
        check(ctx, "ramp", 64, 80, q)


def refused(text, call, *args, **kwargs):
    try:
        call(*args, **kwargs)
    except capi.OchipError as e:
        assert text in str(e), str(e)
        return
    raise AssertionError("not refused: " + text)


def scenario_refusals(ctx):
    for w, h, q, text in ((0, 4, 95, "a raster of 0 x 4"), (4, 0, 95, "a raster of 4 x 0"), (65501, 4, 95, "a raster of 65501 x 4"),
                          (4, 65501, 95, "a raster of 4 x 65501"), (4, 4, 0, "quality 0"), (4, 4, 101, "quality 101")):
        refused(text, host.JpegEncoder, w, h, ctx=ctx, quality=q, on_device=True)
    rgba = to_device(F.rgba_of(F.ramp(40, 24)))
    with host.JpegEncoder(24, 40, ctx=ctx, on_device=True) as e:
        refused("gap: rows 8 to 16 when row 0 is next", e.feed, 8, rgba[8:16])
        e.feed(0, rgba[:20])
        refused("overlap: rows 16 to 24 when row 20 is next", e.feed, 16, rgba[16:24])
        refused("rows 20 to 60 of a raster of 40 rows", e.feed, 20, torch.cat([rgba[20:], rgba[20:]]))
        refused("finish at row 20 of 40", e.finish)
        refused("the capacity is 5", e.collect, 5)
        e.feed(20, rgba[20:])
        got = e.collect() + e.finish()
        refused("after finish", e.feed, 40, rgba[:1])
        refused("finish after finish", e.finish)
        dead = e.h
    same(got, host.encode_jpeg(F.ramp(40, 24)), "the encoder after its refusals")
    L = host.load()
    assert L.och_jpeg_feed(dead, 0, 1, rgba.data_ptr(), 4, 1) == -1  # OCHIP_EINVAL: a dead handle is refused, not followed
    assert "not a live" in L.och_jpeg_last_error().decode()
    assert L.och_jpeg_finish(dead) == -1


def scenario_mosaic(ctx, solve):
    gsd, t, tile_rows = MOSAIC
    g, s, imgs = four_camera_scene(seed=4)
    plan = mosaic_plan(gsd)
    cfg = dict(tile_size=t, blend_transition_radius=10)
    balance = "solve" if solve else None
    dimg = [torch.from_numpy(im).to("cuda:0") for im in imgs]
    with host.OrthoMesh(ctx, [s]) as mesh:
        plain = host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, tile_rows=tile_rows, color_balance=balance)
        f = io.BytesIO()
        out = host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, tile_rows=tile_rows, color_balance=balance, jpeg=f)
        assert isinstance(out, torch.Tensor) and torch.equal(out, plain) and (plain[..., 3] == 255).any()  # the raster unchanged
        same(f.getvalue(), host.encode_jpeg(out, ctx=ctx), "the mosaic's file against encode_jpeg of the returned mosaic")
        fs = io.BytesIO()
        out_s = host.ortho_mosaic_streamed(plan, g, [s], lambda i: imgs[i], mesh, len(imgs), config=cfg, tile_rows=tile_rows,
                                           color_balance=balance, jpeg=fs)
        assert torch.equal(out_s, plain)
        same(fs.getvalue(), f.getvalue(), "the streamed mosaic's file")
    fc = io.BytesIO()
    out_c = host.ortho_mosaic(plan, g, [s], imgs, config=cfg, tile_rows=tile_rows, color_balance=balance, jpeg=fc)
    assert np.array_equal(out_c, out.cpu().numpy())
    same(f.getvalue(), fc.getvalue(), "the mosaic's file against the CPU-route mosaic's")
    same(fc.getvalue(), host.encode_jpeg(out_c), "the CPU-route mosaic's file against encode_jpeg")


def scenarios():
    s = {f"shape_{h}x{w}": (scenario_shape, (h, w)) for h, w in F.SHAPES}
    s.update({c[0]: (scenario_large, c) for c in LARGE})
    s.update(splits=(scenario_splits,), two_encoders=(scenario_two_encoders,), qualities=(scenario_qualities,),
             refusals=(scenario_refusals,), mosaic=(scenario_mosaic, False), mosaic_solve=(scenario_mosaic, True))
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

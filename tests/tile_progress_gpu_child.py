"""The scenarios of test_gpu_tile_progress.py, run in a child process that brings torch up before libochip.so (as
ortho_overviews_gpu_child.py does).  `python tile_progress_gpu_child.py <tests dir> <repo dir>` runs every scenario and
prints one JSON line {scenario: "ok" or the failure's traceback}.  A scenario that ends in a device error ends the run: the
ones after it are reported as not run."""
import json
import sys
import traceback

import numpy as np
import torch

torch.cuda.init()
if __name__ == "__main__":
    sys.path[:0] = sys.argv[1:3]

from layers_fixtures import four_camera_scene  # noqa: E402
from tile_progress_fixtures import (BLEND_CONTENTS, CASES, LAYER_CONTENTS, LAYER_COUNTS, blended, case_id, difference, layers,  # noqa: E402
                                    mosaic_difference, mosaic_order, mosaic_plan, plan_of, slots_of, yardstick)
from opencalibration_amd import capi, host  # noqa: E402

# (gsd, tile_size, tile_rows): 105 x 90 in tiles of 32, bands of 64 and 26 rows; 210 x 180 in tiles of 160 (160 x 160, 50 x
# 160, 160 x 20 and 50 x 20: scales 2, 2, 2 and 1), bands of 160 and 20 rows
MOSAICS = {"105x90_T32": (0.1, 32, 2), "210x180_T160": (0.05, 160, 1)}


def to_device(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()  # the kernel runs on the context's own stream
    return t


def check_band(ctx, plan, t, pass_, pixels, weight, what):
    want = yardstick(plan, pixels, pass_, t, weight=weight)
    cpu = host.ortho_tile_updates(plan, pixels, pass_, tile_size=t, weight=weight)
    d_pixels, d_weight = to_device(pixels), None if weight is None else to_device(weight)
    dev = host.ortho_tile_updates(plan, d_pixels, pass_, tile_size=t, weight=d_weight, ctx=ctx)
    assert difference(dev, want) == "", what
    assert difference(dev, cpu) == "", what
    raw = host.ortho_tile_thumbs(d_pixels, pass_, tile_size=t, weight=d_weight, ctx=ctx)
    assert np.array_equal(raw, slots_of(want, t)), what  # the slots' padding included


def scenario_case(ctx, case, num_layers):
    cols, rows, t = case
    plan = plan_of(cols, rows)
    for content in LAYER_CONTENTS:
        bgra, weight = layers(content, num_layers, rows, cols)
        check_band(ctx, plan, t, 1, bgra, weight, content)
    if num_layers == LAYER_COUNTS[0]:  # the blend pass reads no layers: once per shape
        for content in BLEND_CONTENTS:
            check_band(ctx, plan, t, 2, blended(content, rows, cols), None, content)


def scenario_device_input_equals_host_input(ctx):
    for cols, rows, t in ((300, 130, 128), (260, 129, 129)):
        plan = plan_of(cols, rows)
        bgra, weight = layers("mixed", 2, rows, cols)
        rgba = blended("alpha_mixed", rows, cols)
        for pass_, pixels, w in ((1, bgra, weight), (2, rgba, None)):
            from_host = host.ortho_tile_updates(plan, pixels, pass_, tile_size=t, weight=w, ctx=ctx)  # numpy in, through the device
            from_device = host.ortho_tile_updates(plan, to_device(pixels), pass_, tile_size=t, weight=None if w is None else to_device(w),
                                                  ctx=ctx)
            assert difference(from_host, from_device) == "" and difference(from_host, yardstick(plan, pixels, pass_, t, weight=w)) == ""
            assert np.array_equal(host.ortho_tile_thumbs(pixels, pass_, tile_size=t, weight=w, ctx=ctx),
                                  host.ortho_tile_thumbs(pixels, pass_, tile_size=t, weight=w))


def scenario_object(ctx):
    """the object on the device: two bands of both passes in flight, collected oldest first; the refusals launch nothing"""
    plan, t = plan_of(70, 40), 32
    bgra, weight = layers("mixed", 2, 40, 70)
    rgba = blended("alpha_mixed", 40, 70)
    d_rgba = to_device(rgba)
    top, top_w, rest, rest_w = (to_device(a) for a in (bgra[:, :32], weight[:, :32], bgra[:, 32:], weight[:, 32:]))
    with host.TileProgress(plan, t, 2, ctx=ctx) as p:
        for text, args in (("gap: rows 32 to 40 of pass 2 when row 0 is next", (2, 32, d_rgba[32:])),
                           ("row 16 is not on a tile row", (2, 16, d_rgba[16:])),
                           ("needs the layers' weights", (1, 0, top))):
            try:
                p.feed(*args)
                raise AssertionError("not refused: " + text)
            except capi.OchipError as e:
                assert text in str(e), str(e)
        assert p.pending() == 0
        p.feed(1, 0, top, top_w)
        p.feed(2, 0, d_rgba[:32])
        p.feed(1, 32, rest, rest_w)
        p.feed(2, 32, d_rgba[32:])
        assert p.pending() == 4
        got = [p.collect() for _ in range(4)]
        assert p.pending() == 0
    want = [yardstick(plan, bgra[:, :32], 1, t, 0, weight[:, :32]), yardstick(plan, rgba[:32], 2, t, 0),
            yardstick(plan, bgra[:, 32:], 1, t, 32, weight[:, 32:]), yardstick(plan, rgba[32:], 2, t, 32)]
    for g, x in zip(got, want):
        assert difference(g, x) == ""
    with host.TileProgress(plan, t, 2, ctx=ctx) as p:  # destroyed with a band still in flight
        p.feed(2, 0, d_rgba[:32])
    try:
        host.ortho_tile_thumbs(d_rgba, 2, tile_size=0, ctx=ctx)
        raise AssertionError("tile_size 0 was not refused")
    except capi.OchipError as e:
        assert "tile_size 0" in str(e), str(e)


def scenario_mosaic(ctx, which):
    gsd, t, tile_rows = MOSAICS[which]
    g, s, imgs = four_camera_scene(seed=4)
    plan = mosaic_plan(gsd)
    assert (plan["width"], plan["height"]) == {0.1: (105, 90), 0.05: (210, 180)}[gsd]
    cfg = dict(tile_size=t, blend_transition_radius=10)
    dimg = [torch.from_numpy(im).to("cuda:0") for im in imgs]
    with host.OrthoMesh(ctx, [s]) as mesh:
        plain = host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, tile_rows=tile_rows)
        bands = list(host.ortho_layers_bands(plan, g, [s], dimg, mesh=mesh, tile_rows=tile_rows, config=dict(tile_size=t)))
        assert isinstance(bands[0]["bgra"], np.ndarray) and len(bands) == 2
        resident = []
        out = host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, tile_rows=tile_rows, progress=resident.append)
        assert isinstance(out, torch.Tensor) and torch.equal(out, plain) and (plain[..., 3] == 255).any()  # the raster unchanged
        assert mosaic_order(resident, plan, t, tile_rows, solve=False) == ""  # and every update delivered before return
        assert mosaic_difference(resident, plan, t, out.cpu().numpy(), bands) == ""
        assert {u["scale"] for u in resident} == ({1} if t == 32 else {1, 2})
        assert any((u["thumbnail"][..., 3] == 255).any() for u in resident if u["pass"] == 1)
        streamed = []
        out_s = host.ortho_mosaic_streamed(plan, g, [s], lambda i: imgs[i], mesh, len(imgs), config=cfg, tile_rows=tile_rows,
                                           progress=streamed.append)
        assert torch.equal(out_s, plain) and difference(streamed, resident) == ""
        assert mosaic_order(streamed, plan, t, tile_rows, solve=False) == ""
        only_layers = []
        host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, tile_rows=tile_rows, progress=only_layers.append,
                          progress_passes=(1,))
        assert difference(only_layers, [u for u in resident if u["pass"] == 1]) == ""
        # "solve": pass 1 in the first sweep, pass 2 in the second
        plain_solved = host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, tile_rows=tile_rows, color_balance="solve")
        for run in (lambda cb: host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, tile_rows=tile_rows, color_balance="solve",
                                                 progress=cb),
                    lambda cb: host.ortho_mosaic_streamed(plan, g, [s], lambda i: imgs[i], mesh, len(imgs), config=cfg,
                                                          tile_rows=tile_rows, color_balance="solve", progress=cb)):
            solved = []
            out2 = run(solved.append)
            assert torch.equal(out2, plain_solved)
            assert mosaic_order(solved, plan, t, tile_rows, solve=True) == ""
            assert mosaic_difference(solved, plan, t, out2.cpu().numpy(), bands) == ""
        # the CPU route of the mosaic emits the device's updates
        cpu = []
        out_c = host.ortho_mosaic(plan, g, [s], imgs, config=cfg, tile_rows=tile_rows, progress=cpu.append)
        assert np.array_equal(out_c, plain.cpu().numpy()) and difference(cpu, resident) == ""

        # a callback that raises: the exception arrives, the context stays usable
        def boom(update, seen=[]):
            seen.append(update)
            if len(seen) == 3:
                raise RuntimeError("the callback's own")

        for run in (lambda: host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, tile_rows=tile_rows, progress=boom),):
            try:
                run()
                raise AssertionError("the callback's exception was swallowed")
            except RuntimeError as e:
                assert "the callback's own" in str(e)
        again = []
        out3 = host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, tile_rows=tile_rows, progress=again.append)
        assert torch.equal(out3, plain) and difference(again, resident) == ""
    g.close()


SCENARIOS = {f"case_{case_id(c)}_L{n}": (lambda ctx, c=c, n=n: scenario_case(ctx, c, n)) for c in CASES for n in LAYER_COUNTS}
SCENARIOS.update({
    "device_input_equals_host_input": scenario_device_input_equals_host_input,
    "object": scenario_object,
})
SCENARIOS.update({f"mosaic_{m}": (lambda ctx, m=m: scenario_mosaic(ctx, m)) for m in MOSAICS})

if __name__ == "__main__":
    ctx = capi.Context(0)
    res, device_error = {}, False
    for name, fn in SCENARIOS.items():
        try:
            fn(ctx)
            res[name] = "ok"
        except AssertionError:
            res[name] = traceback.format_exc()
        except Exception:
            res[name] = traceback.format_exc()
            device_error = True
            break
    for name in SCENARIOS:
        res.setdefault(name, "not run: an earlier scenario ended in an error")
    print(json.dumps(res), flush=True)
    if not device_error:
        ctx.close()

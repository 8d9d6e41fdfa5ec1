"""The scenarios of test_gpu_ortho_overviews.py, run in a child process that brings torch up before libochip.so (as
thumbnails_gpu_child.py does).  `python ortho_overviews_gpu_child.py <tests dir> <repo dir> <results.npz>` runs every
scenario, prints one JSON line {scenario: "ok" or the failure's traceback} and stores every level the device computed in
the results file, so that a run under OCHIP_TEST_HOOKS=overview_per_level - the hook is read from the environment, hence a
process of its own - can be compared with the default route's.  A scenario that ends in a device error ends the run: the
ones after it are reported as not run."""
import json
import os
import sys
import traceback

import numpy as np
import torch

torch.cuda.init()
if __name__ == "__main__":
    sys.path[:0] = sys.argv[1:3]

from blend_gpu_child import color_table, small_plan  # noqa: E402
from layers_fixtures import four_camera_scene  # noqa: E402
from ortho_overviews_fixtures import PARTITION_SHAPE, PARTITIONS, cases, fed_in_bands, raster, same  # noqa: E402
from opencalibration_amd import capi, host  # noqa: E402

STORED = {}
PARTITION_CONTENTS = ["alpha_mixed", "nan_random", "large_halves"]
_cpu = {}


def cpu_route(content, w, h):
    """host.ortho_overviews of a content at a shape on the CPU route: computed once, shared, left unchanged"""
    if (content, w, h) not in _cpu:
        _cpu[(content, w, h)] = host.ortho_overviews(raster(content, w, h))
    return _cpu[(content, w, h)]


def to_device(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()  # the builder's kernels run on the context's own stream
    return t


def store(name, levels):
    for k, l in enumerate(levels):
        STORED[f"{name}/{k + 1}"] = l.view(np.uint32) if l.dtype == np.float32 else l


def scenario_case(ctx, name, content, w, h):
    got = [l.cpu().numpy() for l in host.ortho_overviews(to_device(raster(content, w, h)), ctx)]
    want = cpu_route(content, w, h)
    assert len(got) == len(want)
    for k, (g, x) in enumerate(zip(got, want)):
        assert same(g, x), (k + 1, int((g.view(np.uint32) != x.view(np.uint32)).sum()) if g.shape == x.shape else g.shape)
    store(name, got)


def scenario_partition(ctx, content, partition):
    w, h = PARTITION_SHAPE
    got = fed_in_bands(host, raster(content, w, h), PARTITIONS[partition], ctx=ctx, to_device=to_device)
    for k, (g, x) in enumerate(zip(got, cpu_route(content, w, h))):
        assert same(g, x), k + 1
    store(f"partition_{partition}_{content}", got)


def scenario_device_input_equals_host_input(ctx):
    for content in ("alpha_half", "nan_random"):
        for w, h in ((130, 67), (129, 200)):
            level0 = raster(content, w, h)
            from_host = host.ortho_overviews(level0, ctx)  # numpy in and out through the device
            from_device = [l.cpu().numpy() for l in host.ortho_overviews(to_device(level0), ctx)]
            banded = fed_in_bands(host, level0, [33, h - 33], ctx=ctx)  # host bands through the device, an odd first band
            assert len(from_host) == len(from_device) > 0
            for a, b, c, d in zip(from_host, from_device, banded, cpu_route(content, w, h)):
                assert isinstance(a, np.ndarray) and same(a, b) and same(a, c) and same(a, d)


def mosaic_scene():
    """blend_gpu_child.py's scenario_device_tensor_mosaic: 105 x 90, bands of 64 and 26 rows, six levels"""
    g, s, imgs = four_camera_scene(seed=4)
    plan = small_plan(0.1)
    assert (plan["width"], plan["height"]) == (105, 90)
    return g, s, imgs, plan, dict(tile_size=32, blend_transition_radius=10)


def check_mosaic_levels(ctx, name, out, over, plain, whole_dsm):
    assert torch.equal(out, plain) and (plain[..., 3] == 255).any()
    assert len(over["rgba"]) == len(over["dsm"]) == 6
    want_rgba = host.ortho_overviews(plain, ctx)
    want_dsm = host.ortho_overviews(whole_dsm, ctx)
    cpu_rgba, cpu_dsm = host.ortho_overviews(plain.cpu().numpy()), host.ortho_overviews(whole_dsm.cpu().numpy())
    for k in range(6):
        assert torch.equal(over["rgba"][k], want_rgba[k]), k + 1
        assert same(over["dsm"][k].cpu().numpy(), want_dsm[k].cpu().numpy()), k + 1
        assert same(over["rgba"][k].cpu().numpy(), cpu_rgba[k]) and same(over["dsm"][k].cpu().numpy(), cpu_dsm[k]), k + 1
    assert not torch.isnan(over["dsm"][0]).all()
    store(name + "_rgba", [l.cpu().numpy() for l in over["rgba"]])
    store(name + "_dsm", [l.cpu().numpy() for l in over["dsm"]])


def scenario_mosaic(ctx, streamed, color_balance):
    g, s, imgs, plan, cfg = mosaic_scene()
    if color_balance == "tables":
        color_balance = color_table(g, [s], 6)
    dimg = [torch.from_numpy(im).to("cuda:0") for im in imgs]
    with host.OrthoMesh(ctx, [s]) as mesh:
        plain = host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, color_balance=color_balance, tile_rows=2)
        assert isinstance(plain, torch.Tensor)  # overviews=False: the return value it always had
        if streamed:
            out, over = host.ortho_mosaic_streamed(plan, g, [s], lambda i: imgs[i], mesh, len(imgs), config=cfg,
                                                   color_balance=color_balance, tile_rows=2, overviews=True)
        else:
            out, over = host.ortho_mosaic(plan, g, [s], dimg, mesh=mesh, config=cfg, color_balance=color_balance, tile_rows=2,
                                          overviews=True)
        whole_dsm = host.dsm_render(plan, [s], mesh=mesh)
        if not isinstance(whole_dsm, torch.Tensor):
            whole_dsm = to_device(whole_dsm)
        check_mosaic_levels(ctx, f"mosaic_{int(streamed)}_{color_balance == 'solve'}", out, over, plain, whole_dsm)
    g.close()


def scenario_cpu_mosaic(ctx):
    """the CPU route of the mosaic feeds CPU builders: the same levels as ortho_overviews of its results"""
    g, s, imgs, plan, cfg = mosaic_scene()
    out, over = host.ortho_mosaic(plan, g, [s], imgs, config=cfg, tile_rows=2, overviews=True)
    for got, want in zip(over["rgba"], host.ortho_overviews(out)):
        assert same(got, want)
    for got, want in zip(over["dsm"], host.ortho_overviews(host.dsm_render(plan, [s]))):
        assert same(got, want)
    g.close()


def scenario_refusals(ctx):
    level0 = to_device(raster("alpha_half", 20, 30))
    with host.OrthoOverviews(host.OVERVIEW_RGBA8, 20, 30, ctx=ctx, on_device=True) as b:
        b.feed(0, level0[0:10])
        for row0, rows, text in ((12, 8, "gap: rows 12 to 20"), (8, 8, "overlap: rows 8 to 16"), (10, 21, "rows 10 to 31")):
            try:
                b.feed(row0, torch.zeros((rows, 20, 4), dtype=torch.uint8, device="cuda:0"))
                raise AssertionError("not refused: " + text)
            except capi.OchipError as e:
                assert text in str(e), str(e)
        try:
            b.finish()
            raise AssertionError("finish before the last row was not refused")
        except capi.OchipError as e:
            assert "rows 0 to 10 of 30" in str(e), str(e)
        b.feed(10, level0[10:30])
        got = [l.cpu().numpy() for l in b.finish()]
        try:
            b.feed(30, level0[0:1])
            raise AssertionError("a feed after finish was not refused")
        except capi.OchipError as e:
            assert "after finish" in str(e), str(e)
    for g, x in zip(got, cpu_route("alpha_half", 20, 30)):
        assert same(g, x)


SCENARIOS = {name: (lambda ctx, c=(name, content, w, h): scenario_case(ctx, *c)) for name, content, w, h in cases()}
SCENARIOS.update({f"partition_{p}_{c}": (lambda ctx, c=c, p=p: scenario_partition(ctx, c, p))
                  for p in sorted(PARTITIONS) for c in PARTITION_CONTENTS})
SCENARIOS.update({
    "device_input_equals_host_input": scenario_device_input_equals_host_input,
    "refusals": scenario_refusals,
    "mosaic": lambda ctx: scenario_mosaic(ctx, False, "tables"),
    "mosaic_streamed": lambda ctx: scenario_mosaic(ctx, True, "tables"),
    "mosaic_solve": lambda ctx: scenario_mosaic(ctx, False, "solve"),
    "mosaic_cpu_route": scenario_cpu_mosaic,
})

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
    res["hooks"] = os.environ.get("OCHIP_TEST_HOOKS", "")
    np.savez(sys.argv[3], **STORED)
    print(json.dumps(res), flush=True)
    if not device_error:
        ctx.close()

"""The scenarios of test_gpu_ortho_stream.py, run in a child process that brings torch up before libochip.so (as
layers_gpu_child.py does).  `python ortho_stream_gpu_child.py <tests dir> <repo dir>` runs every scenario and prints one
JSON line {scenario: "ok" or the failure's traceback}."""
import json
import sys
import traceback

import numpy as np
import torch

torch.cuda.init()
if __name__ == "__main__":
    sys.path[:0] = sys.argv[1:3]

from ortho_stream_fixtures import (AHEAD, BAND_SET_SCENES, LATE, band_cameras_raw, plan_restated, scene_overflow, sets_of,  # noqa: E402
                                   strip_scene)
from opencalibration_amd import capi, host  # noqa: E402

_strip = {}


def strip(ctx):
    """the strip scene, its images on the device and page-locked on the host, and the all-resident render of every band:
    made once, shared by the scenarios, left unchanged"""
    if not _strip:
        g, s, imgs, plan, cfg = strip_scene()
        mesh = host.OrthoMesh(ctx, [s])
        dev = [torch.from_numpy(im).to("cuda:0") for im in imgs]
        pinned = [torch.from_numpy(im).pin_memory() for im in imgs]
        resident = list(host.ortho_layers_bands(plan, g, [s], dev, mesh=mesh, tile_rows=1, config=cfg))
        used = host.ortho_band_cameras(plan, g, [s], config=cfg, ctx=ctx)
        _strip.update(g=g, s=s, imgs=imgs, plan=plan, cfg=cfg, mesh=mesh, dev=dev, pinned=pinned, resident=resident,
                      sets=sets_of(used))
    return _strip


def assert_same(a, b):
    assert np.array_equal(a["bgra"], b["bgra"])
    assert np.array_equal(a["camera_id"], b["camera_id"])
    assert np.array_equal(a["weight"].view(np.uint32), b["weight"].view(np.uint32))
    assert len(a["correspondences"]) == len(b["correspondences"])
    assert a["correspondences"].tobytes() == b["correspondences"].tobytes()


def scenario_band_sets(ctx, name):
    g, s, _, plan, cfg = BAND_SET_SCENES[name]()
    for tile_rows in (1, 2):
        cpu = host.ortho_band_cameras(plan, g, [s], tile_rows=tile_rows, config=cfg)
        dev = host.ortho_band_cameras(plan, g, [s], tile_rows=tile_rows, config=cfg, ctx=ctx)
        assert cpu.any() and np.array_equal(dev, cpu)
    g.close()


def scenario_band_sets_overflow(ctx):
    cams, plan = scene_overflow()
    cpu = band_cameras_raw(cams, plan, 16)
    assert cpu.any(1).all() and np.array_equal(band_cameras_raw(cams, plan, 16, ctx=ctx), cpu)


def stream_equals_resident(ctx, tight):
    sc = strip(ctx)
    sets = sc["sets"]
    capacity = max(len(s) for s in sets) if tight else max(len(a | b) for a, b in zip(sets, sets[1:]))
    assert capacity < len(sc["imgs"])  # evictions happen
    with host.OrthoStream(sc["plan"], sc["g"], [sc["s"]], capacity, mesh=sc["mesh"], config=sc["cfg"]) as stream:
        planned = [stream.loads(k) for k in range(stream.num_bands)]
        assert planned == plan_restated(sets, capacity)[0]
        assert any(l[2] == LATE for band in planned for l in band) == tight
        assert sum(len(b) for b in planned) >= len(sc["imgs"])
        for sweep in range(2):
            for k in range(stream.num_bands):
                for cam, _, _ in (stream.loads(k) if k == 0 else stream.loads(k, LATE)):
                    stream.upload(k, cam, sc["pinned"][cam])
                if k + 1 < stream.num_bands:
                    for cam, _, _ in stream.loads(k + 1, AHEAD):
                        stream.upload(k + 1, cam, sc["pinned"][cam])
                assert_same(stream.render(k), sc["resident"][k])
            if sweep == 0:
                stream.rewind()
    assert (sc["resident"][0]["bgra"][..., 3] == 255).any() and sum(len(b["correspondences"]) for b in sc["resident"]) > 0


def scenario_ordering_contract(ctx):
    sc = strip(ctx)
    sets, pinned = sc["sets"], sc["pinned"]
    capacity = max(len(a | b) for a, b in zip(sets, sets[1:]))

    def refused(what, fn, *args):
        try:
            fn(*args)
        except capi.OchipError as e:
            assert what in str(e), str(e)
            return
        raise AssertionError(f"not refused: {what}")

    refused("the capacity is 2", host.OrthoStream, sc["plan"], sc["g"], [sc["s"]], 2, sc["mesh"], 1, sc["cfg"])
    with host.OrthoStream(sc["plan"], sc["g"], [sc["s"]], capacity, mesh=sc["mesh"], config=sc["cfg"]) as stream:
        refused("not uploaded", stream.render, 0)
        refused("ascending", stream.render, 1)
        k = next(k for k in range(2, stream.num_bands) if stream.loads(k))
        cam = stream.loads(k)[0][0]
        refused(f"waits for render({k - 2})", stream.upload, k, cam, pinned[cam])
        refused("rewind", stream.rewind)
        first = stream.loads(0)[0][0]
        stream.upload(0, first, pinned[first])
        refused("uploaded already", stream.upload, 0, first, pinned[first])
        refused("not uploaded", stream.render, 0)


def mosaic(ctx, color_balance):
    sc = strip(ctx)
    sets = sc["sets"]
    capacity = max(len(a | b) for a, b in zip(sets, sets[1:]))
    cfg = dict(sc["cfg"], correspondence_subsample=5)
    want = host.ortho_mosaic(sc["plan"], sc["g"], [sc["s"]], sc["dev"], mesh=sc["mesh"], config=cfg, color_balance=color_balance)
    fetched = []

    def fetch(i):
        fetched.append(i)
        return sc["pinned"][i] if i % 2 else sc["imgs"][i]  # page-locked tensors and plain numpy arrays

    got = host.ortho_mosaic_streamed(sc["plan"], sc["g"], [sc["s"]], fetch, sc["mesh"], capacity, config=cfg,
                                     color_balance=color_balance)
    assert torch.equal(got, want) and (want[..., 3] == 255).any()
    assert set(fetched) == set(range(len(sc["imgs"])))


SCENARIOS = {f"band_sets_{name}": (lambda ctx, name=name: scenario_band_sets(ctx, name)) for name in sorted(BAND_SET_SCENES)}
SCENARIOS.update({
    "band_sets_overflow": scenario_band_sets_overflow,
    "streamed_equals_resident_ahead_only": lambda ctx: stream_equals_resident(ctx, False),
    "streamed_equals_resident_late_loads": lambda ctx: stream_equals_resident(ctx, True),
    "ordering_contract": scenario_ordering_contract,
    "mosaic_without_color_balance": lambda ctx: mosaic(ctx, None),
    "mosaic_solve": lambda ctx: mosaic(ctx, "solve"),
})

if __name__ == "__main__":
    ctx = capi.Context(0)
    res = {}
    for name, fn in SCENARIOS.items():
        try:
            fn(ctx)
            res[name] = "ok"
        except Exception:
            res[name] = traceback.format_exc()
    if _strip:
        _strip["mesh"].close()
    ctx.close()
    print(json.dumps(res))

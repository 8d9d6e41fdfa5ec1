"""The scenarios of test_gpu_thumbnails.py, run in a child process that brings torch up before libochip.so (as
ortho_stream_gpu_child.py does).  `python thumbnails_gpu_child.py <tests dir> <repo dir>` runs every scenario and prints
one JSON line {scenario: "ok" or the failure's traceback}.  A scenario that ends in a device error ends the run: the ones
after it are reported as not run."""
import json
import sys
import traceback

import numpy as np
import torch

torch.cuda.init()
if __name__ == "__main__":
    sys.path[:0] = sys.argv[1:3]

from ortho_fixtures import DOWN  # noqa: E402
from thumbnail_fixtures import SHAPES, cpu_route, images  # noqa: E402
from opencalibration_amd import capi, host  # noqa: E402


def scenario_shape(ctx, name):
    w, h, batch = SHAPES[name]
    got = host.image_thumbnails(images(name), ctx)
    assert got.shape == (batch,) + host.thumbnail_size(w, h) + (3,)
    assert np.array_equal(got, cpu_route(name))


def scenario_table_equals_function(ctx):
    rng = np.random.default_rng(24)
    ramp = np.arange(256, dtype=np.uint32)
    edges = []  # the 12 edges of the colour cube: one channel runs, the other two sit at 0 or 255
    for run in range(3):
        a, b = [c for c in range(3) if c != run]
        for va in (0, 255):
            for vb in (0, 255):
                edges.append(ramp << (8 * run) | np.uint32(va << (8 * a)) | np.uint32(vb << (8 * b)))
    codes = np.concatenate([rng.integers(0, 1 << 24, 1 << 20, dtype=np.uint32), ramp * np.uint32(0x010101)] + edges)
    assert len(codes) == (1 << 20) + 256 + 12 * 256
    got, fill_ms = ctx.lab_table(codes)
    assert fill_ms > 0
    bgr = np.stack([codes & 255, codes >> 8 & 255, codes >> 16 & 255], -1).astype(np.uint8)
    lab = host.lab_convert(bgr, "bgr2lab8").astype(np.uint32)
    assert np.array_equal(got, lab[:, 0] | lab[:, 1] << 8 | lab[:, 2] << 16)


def small_survey(ctx):
    """a 3 x 2 grid of 400 x 300 synthetic views in HBM: (pointer, positions, orientations, model)"""
    w, h, f = 400, 300, 300.0
    pos = np.array([(c * 25.0 + 0.3 * r, r * 45.0 - 0.2 * c, 100.0) for r in range(2) for c in range(3)], np.float64)
    ori = np.tile(DOWN, (len(pos), 1))
    ptr = ctx.synth_views(pos, ori, w, h, f, (w / 2, h / 2), (0.0, 0.0), 7.0, (-500.0, -500.0), seed=3)
    return ptr, pos, ori, np.array([f, w / 2, h / 2, 0, 0, 0, 0, 0, w, h], np.float64)


def scenario_device_input_equals_host_input(ctx):
    ptr, pos, _, _ = small_survey(ctx)
    n, w, h = len(pos), 400, 300
    back = np.stack([ctx.synth_views_read(ptr, i, w, h) for i in range(n)])
    from_device = host.image_thumbnails(ptr, ctx, device_shape=(n, h, w))
    ctx.synth_views_free(ptr)
    assert len(np.unique(back)) > 16
    assert np.array_equal(from_device, host.image_thumbnails(back, ctx))
    assert np.array_equal(from_device, host.image_thumbnails(back))


def scenario_preview_from_pixels(ctx):
    ptr, pos, ori, model = small_survey(ctx)
    n, w, h = len(pos), 400, 300
    back = np.stack([ctx.synth_views_read(ptr, i, w, h) for i in range(n)])
    surface = host.rebuild_mesh(pos)
    surface.set_heights(np.zeros(len(surface.arrays()["vertices"])))
    g = host.Graph()
    g.load_images(ctx, ptr, g.add_model(model), pos, max_keypoints=2000, device_shape=(n, h, w), thumbnails=True)
    ctx.synth_views_free(ptr)
    g.set_orientations(ori)
    got = host.orthomosaic_thumbnail(g, [surface], ctx)
    g2 = host.Graph()
    m2 = g2.add_model(model)
    for p in pos:
        g2.add_image(np.zeros((0, 2)), np.zeros(0, np.float32), np.zeros((0, 8), np.uint64), 0, m2, p)
    g2.set_orientations(ori)
    for i, t in enumerate(host.image_thumbnails(back)):
        g2.set_thumbnail(i, t)
    want = host.orthomosaic_thumbnail(g2, [surface], ctx)
    assert g.node_ids == g2.node_ids
    g.close(), g2.close()
    assert np.array_equal(got["rgba"], want["rgba"]) and np.array_equal(got["ids"], want["ids"])
    assert (got["rgba"][..., 3] == 255).mean() > 0.2 and len(np.unique(got["ids"])) >= n


SCENARIOS = {name: (lambda ctx, name=name: scenario_shape(ctx, name)) for name in SHAPES}
SCENARIOS.update({
    "table_equals_function": scenario_table_equals_function,
    "device_input_equals_host_input": scenario_device_input_equals_host_input,
    "preview_from_pixels": scenario_preview_from_pixels,
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
    print(json.dumps(res), flush=True)
    if not device_error:
        ctx.close()

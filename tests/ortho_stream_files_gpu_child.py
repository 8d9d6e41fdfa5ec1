"""The scenarios of test_gpu_ortho_stream_files.py, run in a child process that brings torch up before libochip.so (as
ortho_stream_gpu_child.py does) and holds one capi.Context(0).  `python ortho_stream_files_gpu_child.py <tests dir> <repo
dir>` runs every scenario and prints one JSON line {scenario: "ok" or the failure's traceback}.  A scenario that ends in
anything but a failed assertion ends the run: the scenarios behind it are reported as not run, and nothing more is started
on the device.  No scenario feeds a damaged scan to a kernel (DESIGN.md section 4.18's rule)."""
import json
import sys
import traceback

import numpy as np
import torch

torch.cuda.init()
if __name__ == "__main__":
    sys.path[:0] = sys.argv[1:3]

import ortho_stream_files_fixtures as X  # noqa: E402
from opencalibration_amd import capi, host  # noqa: E402

_dev = {}


def assert_same(a, b):
    assert np.array_equal(a["bgra"], b["bgra"])
    assert np.array_equal(a["camera_id"], b["camera_id"])
    assert np.array_equal(a["weight"].view(np.uint32), b["weight"].view(np.uint32))
    assert len(a["correspondences"]) == len(b["correspondences"])
    assert a["correspondences"].tobytes() == b["correspondences"].tobytes()


def two_sweeps(stream, how_of, render):
    first = X.sweep(stream, how_of(stream), render)
    stream.rewind()
    return first + X.sweep(stream, how_of(stream), render)


def device(ctx):
    """the scene's mesh, the device's own heights and the decoded images page-locked: made once, left unchanged"""
    if not _dev:
        sc = X.scene()
        mesh = host.OrthoMesh(ctx, [sc["s"]])
        dsm = host.dsm_render(sc["plan"], [sc["s"]], mesh=mesh)
        dsm = dsm if isinstance(dsm, np.ndarray) else dsm.cpu().numpy()
        _dev.update(sc, mesh=mesh, dev_dsm=dsm, pinned=[torch.from_numpy(im).pin_memory() for im in sc["imgs"]], yardstick={})
    return _dev


def open_stream(d, capacity, on_device=True):
    return host.OrthoStream(d["plan"], d["g"], [d["s"]], capacity, mesh=d["mesh"] if on_device else None, config=d["cfg"])


def yardstick(d, capacity):
    """two sweeps of the device stream through upload() of the host-decoded pixels"""
    if capacity not in d["yardstick"]:
        with open_stream(d, capacity) as stream:
            d["yardstick"][capacity] = two_sweeps(stream, lambda st: X.by_upload(st, d["pinned"]), stream.render)
        assert (d["yardstick"][capacity][0]["bgra"][..., 3] == 255).any()
        assert sum(len(b["correspondences"]) for b in d["yardstick"][capacity]) > 0
    return d["yardstick"][capacity]


def files_equal_upload(ctx, capacity):
    d = device(ctx)
    want = yardstick(d, capacity)
    with open_stream(d, capacity) as stream:
        loads = [stream.loads(k) for k in range(stream.num_bands)]
        assert any(l[2] == X.LATE for b in loads for l in b) == (capacity == X.TIGHT)
        got = two_sweeps(stream, lambda st: X.by_files(st, d["files"]), stream.render)
    assert len(got) == len(want) == 2 * len(d["sets"])
    for a, b in zip(got, want):
        assert_same(a, b)
    # and the CPU route from the same files, on the device's own heights
    with open_stream(d, capacity, on_device=False) as stream:
        cpu = two_sweeps(stream, lambda st: X.by_files(st, d["files"]), lambda k: stream.render(k, dsm=d["dev_dsm"][k * 64:(k + 1) * 64]))
    for a, b in zip(got, cpu):
        assert_same(a, b)


def scenario_mixed_band(ctx):
    d = device(ctx)
    for capacity in (X.TIGHT, X.ROOMY):
        with open_stream(d, capacity) as stream:
            got = two_sweeps(stream, lambda st: X.by_both(st, d["pinned"], d["files"]), stream.render)
        for a, b in zip(got, yardstick(d, capacity)):
            assert_same(a, b)


def scenario_orientation_3(ctx):
    d = device(ctx)
    cam = 4
    files = list(d["files"])
    files[cam] = X.with_exif(files[cam], 3)
    imgs = list(d["imgs"])
    imgs[cam] = host.decode_jpeg(files[cam])  # the host loops
    assert np.array_equal(imgs[cam], d["imgs"][cam][::-1, ::-1])
    with open_stream(d, X.TIGHT) as stream:
        got = two_sweeps(stream, lambda st: X.by_files(st, files), stream.render)
    with open_stream(d, X.TIGHT) as stream:
        want = two_sweeps(stream, lambda st: X.by_upload(st, imgs), stream.render)
    for a, b in zip(got, want):
        assert_same(a, b)
    assert any(not np.array_equal(a["bgra"], b["bgra"]) for a, b in zip(want, yardstick(d, X.TIGHT)))  # the turn shows


def mosaic(ctx, color_balance):
    d = device(ctx)
    dev = [torch.from_numpy(im).to("cuda:0") for im in d["imgs"]]
    want = host.ortho_mosaic(d["plan"], d["g"], [d["s"]], dev, mesh=d["mesh"], config=d["cfg"], color_balance=color_balance)
    got = host.ortho_mosaic_streamed(d["plan"], d["g"], [d["s"]], None, d["mesh"], X.TIGHT, config=d["cfg"], color_balance=color_balance,
                                     files=d["files"])
    assert torch.equal(got, want) and (want[..., 3] == 255).any()


def scenario_refusals(ctx):
    """every refusal on one device stream: none launches or marks anything, so render(0) is still refused with all six of
    band 0's loads pending, and the stream then gives the yardstick's bands"""
    d = device(ctx)
    files, pinned = d["files"], d["pinned"]
    band0 = [6, 7, 8, 9, 10, 11]

    def refused(what, fn, *args):
        try:
            fn(*args)
        except capi.OchipError as e:
            assert what in str(e), str(e)
            return
        raise AssertionError(f"not refused: {what}")

    def with_file(cam, bad):
        return [bad if c == cam else files[c] for c in band0]

    with open_stream(d, X.TIGHT) as stream:
        assert [l[0] for l in stream.loads(0)] == band0
        refused("camera 0 is no planned load of band 0", stream.upload_jpegs, 0, [6, 7, 0], [files[6], files[7], files[0]])
        refused("camera 6 appears twice", stream.upload_jpegs, 0, [6, 7, 6], [files[6], files[7], files[6]])
        refused("ahead load of camera 4 for band 2 waits for render(0)", stream.upload_jpegs, 2, [4, 5], [files[4], files[5]])
        refused("camera 7 has no file", stream.upload_jpegs, 0, [6, 7], [files[6], None])
        refused("file of camera 10 is unsupported", stream.upload_jpegs, 0, band0, with_file(10, X.unsupported_file(d, 10)))
        assert stream.jpeg_status == ["ok"] * 4 + ["unsupported", "ok"]
        refused("file of camera 8 is corrupt", stream.upload_jpegs, 0, band0, with_file(8, X.corrupt_header_file(d, 8)))
        refused("file of camera 7 decodes to 160 x 120, the camera's images are 150 x 110", stream.upload_jpegs, 0, band0,
                with_file(7, files[6]))
        refused("file of camera 7 decodes to 110 x 150, the camera's images are 150 x 110", stream.upload_jpegs, 0, band0,
                with_file(7, X.with_exif(files[7], 6)))
        refused("render: 6 planned loads of band 0 are not uploaded", stream.render, 0)
        stream.upload(0, 6, pinned[6])
        refused("camera 6 of band 0 is uploaded already", stream.upload_jpegs, 0, [7, 6], [files[7], files[6]])
        refused("render: 5 planned loads of band 0 are not uploaded", stream.render, 0)
        assert stream.upload_jpegs(0, band0[1:], [files[c] for c in band0[1:]]) == ["ok"] * 5
        order = X.feed_order(stream)
        by_files = X.by_files(stream, files)
        by_files(1, [cam for b, cam in order[0][1] if b == 1])
        bands = [stream.render(0)]
        for k, loads in order[1:]:
            for b in sorted({b for b, _ in loads}):
                by_files(b, [cam for bb, cam in loads if bb == b])
            bands.append(stream.render(k))
    for a, b in zip(bands, yardstick(d, X.TIGHT)):
        assert_same(a, b)


SCENARIOS = {
    "files_equal_upload_late_loads": lambda ctx: files_equal_upload(ctx, X.TIGHT),
    "files_equal_upload_ahead_only": lambda ctx: files_equal_upload(ctx, X.ROOMY),
    "mixed_band": scenario_mixed_band,
    "orientation_3": scenario_orientation_3,
    "mosaic_without_color_balance": lambda ctx: mosaic(ctx, None),
    "mosaic_solve": lambda ctx: mosaic(ctx, "solve"),
    "refusals": scenario_refusals,
}

if __name__ == "__main__":
    ctx = capi.Context(0)
    res = {}
    for name, fn in SCENARIOS.items():
        try:
            fn(ctx)
            res[name] = "ok"
        except AssertionError:
            res[name] = traceback.format_exc()
        except Exception:
            res[name] = traceback.format_exc()
            break
    for name in SCENARIOS:
        res.setdefault(name, "not run: a scenario before it ended in an error")
    print(json.dumps(res), flush=True)
    if all(v == "ok" for v in res.values()):  # after an error nothing more is asked of the device
        _dev["mesh"].close()
        ctx.close()

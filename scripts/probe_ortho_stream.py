"""The layered render with streamed source images on C3 geometry: the scene of probe_ortho_layers.py (synth.make_grid(40,
25), 1 000 views), the views read back into page-locked host memory and streamed through 256 device slots band by band
(host.OrthoStream), one 1 024-row tile row per band.  Prints one JSON line: the band-set launch's time, the sets' sizes,
the bytes uploaded and whether that is one upload per image, the streamed layer pass (best of 3 cold sweeps, with the
range) and the two references measured in the same process - the all-resident layer pass and a plain page-locked
host-to-device copy of the same bytes on the copy stream - then how far the streamed time lies above the larger of the
two, and the per-band timeline (upload end on the device against render start and end on the host, ms since the sweep
began).  --views NX NY: another grid.  --capacity N.  Needs the GPU."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opencalibration_amd import capi, host, pipeline, synth  # noqa: E402


def option(name, count, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        return [int(v) for v in sys.argv[i + 1:i + 1 + count]]
    return default


def main():
    import torch

    torch.cuda.init()  # torch's HIP runtime comes up before libochip.so is loaded (as in bench.py)
    nx, ny = option("--views", 2, [40, 25])
    capacity, = option("--capacity", 1, [256])
    grid = synth.make_grid(nx, ny, feats=16)
    pos = np.ascontiguousarray(grid.position, np.float64)
    rng = np.random.default_rng(0)
    surface = host.rebuild_mesh(pos)
    v = surface.arrays()["vertices"]
    surface.set_heights(v[:, 2] - grid.meta.get("height", 100.0) + rng.uniform(-2, 2, len(v)))
    g = host.Graph()
    m = g.add_model(np.asarray(grid.model, np.float64))
    for p in pos:
        g.add_image(np.zeros((0, 2)), np.zeros(0, np.float32), np.zeros((0, 8), np.uint64), 0, m, p)
    g.set_orientations(np.ascontiguousarray(grid.orientation, np.float64))
    ctx = capi.Context(0)
    W_img, H_img = int(grid.model[8]), int(grid.model[9])
    image_bytes = W_img * H_img * 3
    views, _ = pipeline.synthetic_views(ctx, grid)
    ptrs = [int(views) + i * image_bytes for i in range(len(pos))]
    plan = host.dsm_plan(g, [surface])
    W, H = plan["width"], plan["height"]
    cfg = host.LAYERS_CONFIG
    T, L = cfg["tile_size"], cfg["num_layers"]
    out = dict(images=len(pos), image_size=[W_img, H_img], device=ctx.device_info()["name"], width=W, height=H, layers=L,
               tile_size=T, bands=-(-H // T), capacity=capacity)
    mesh = host.OrthoMesh(ctx, [surface])
    bufs = dict(bgra=torch.empty((L, T, W, 4), dtype=torch.uint8, device="cuda:0"),
                camera_id=torch.empty((L, T, W), dtype=torch.int64, device="cuda:0"),
                weight=torch.empty((L, T, W), dtype=torch.float32, device="cuda:0"))

    def band_out(rows):  # contiguous (L, rows, ...) views of the band buffers
        return {k: t.view(-1)[:t[:, :rows].numel()].view(t[:, :rows].shape) for k, t in bufs.items()}

    # reference 1: every image resident (probe_ortho_layers.py's loop)
    def render_resident():
        for row0 in range(0, H, T):
            host.ortho_layers(plan, g, [surface], ptrs, mesh=mesh, row0=row0, tile_rows=1, out=band_out(min(T, H - row0)))
        torch.cuda.synchronize()

    render_resident()  # warm-up
    resident = []
    for _ in range(3):
        t0 = time.perf_counter()
        render_resident()
        resident.append(time.perf_counter() - t0)

    # the band sets: one launch for the whole raster
    host.ortho_band_cameras(plan, g, [surface], ctx=ctx)
    sets_s = []
    for _ in range(3):
        t0 = time.perf_counter()
        used = host.ortho_band_cameras(plan, g, [surface], ctx=ctx)
        sets_s.append(time.perf_counter() - t0)
    sizes = used.sum(1)
    out.update(band_sets_s=min(sets_s), band_sets_s_all=sets_s, set_size_min=int(sizes.min()), set_size_median=float(np.median(sizes)),
               set_size_max=int(sizes.max()), cameras_in_any_set=int(used.any(0).sum()))

    # the views in page-locked host memory, in blocks of 100 images
    blocks, releases = [], []
    t0 = time.perf_counter()
    for first in range(0, len(pos), 100):
        arr, release = ctx.host_array((min(100, len(pos) - first), H_img, W_img, 3))
        for j in range(len(arr)):
            ctx.synth_views_read_into(views, first + j, W_img, H_img, arr[j])
        blocks.append(arr)
        releases.append(release)
    out.update(read_back_s=time.perf_counter() - t0)

    def image(i):
        return blocks[i // 100][i % 100]

    # the streamed pass: a new stream per timed sweep, so that every sweep starts with empty slots
    def sweep(timeline):
        with host.OrthoStream(plan, g, [surface], capacity, mesh=mesh, tile_rows=1) as stream:
            uploads = 0
            t0 = time.perf_counter()
            for k in range(stream.num_bands):
                n_late = n_ahead = 0
                for cam, _, _ in (stream.loads(k) if k == 0 else stream.loads(k, host.LOAD_LATE)):
                    stream.upload(k, cam, image(cam))
                    n_late += 1
                if k + 1 < stream.num_bands:
                    for cam, _, _ in stream.loads(k + 1, host.LOAD_AHEAD):
                        stream.upload(k + 1, cam, image(cam))
                        n_ahead += 1
                uploads += n_late + n_ahead
                start = time.perf_counter()
                stream.render(k, out=band_out(min(T, H - k * T)))
                end = time.perf_counter()
                timeline.append(dict(band=k, cameras=len(stream.band_cameras(k)), late_uploads_before=n_late,
                                     ahead_uploads_before=n_ahead, render_start_ms=(start - t0) * 1e3, render_end_ms=(end - t0) * 1e3))
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
            for row in timeline:
                row["upload_end_ms"] = stream.upload_end_ms(row["band"])
        return total, uploads

    sweep([])  # warm-up: the slot block enters the context's pool
    streamed, timeline = [], None
    for _ in range(3):
        rows = []
        s, uploads = sweep(rows)
        if not streamed or s < min(streamed):
            timeline = rows
        streamed.append(s)
    out.update(uploads=uploads, uploaded_bytes=uploads * image_bytes, one_upload_per_image=bool(uploads == int(used.any(0).sum())))

    # reference 2: the same bytes from the same page-locked memory into 8 slots on the copy stream, nothing else running
    lib = capi.load()
    lib.ochip_image_slots_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]
    lib.ochip_image_slots_upload.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
    lib.ochip_image_slots_mark.argtypes = [C.c_void_p, C.c_uint32]
    lib.ochip_image_slots_wait.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
    lib.ochip_image_slots_destroy.argtypes = [C.c_void_p]
    lib.ochip_image_slots_destroy.restype = None
    slots = C.c_void_p()
    if lib.ochip_image_slots_create(ctx.h, 8, image_bytes, 1, C.byref(slots)) != 0:
        raise capi.OchipError("ochip_image_slots_create failed")
    plain = []
    for _ in range(3):
        t0 = time.perf_counter()
        for i in range(uploads):
            if lib.ochip_image_slots_upload(slots, i % 8, image(i % len(pos)).ctypes.data, image_bytes) != 0:
                raise capi.OchipError("ochip_image_slots_upload failed")
        if lib.ochip_image_slots_mark(slots, 0) != 0 or lib.ochip_image_slots_wait(slots, 0, 1) != 0:
            raise capi.OchipError("ochip_image_slots_mark / wait failed")
        plain.append(time.perf_counter() - t0)
    lib.ochip_image_slots_destroy(slots)

    floor = max(min(resident), min(plain))
    out.update(resident_s=min(resident), resident_s_all=resident, plain_copy_s=min(plain), plain_copy_s_all=plain,
               plain_copy_gb_per_s=uploads * image_bytes / min(plain) / 1e9, streamed_s=min(streamed), streamed_s_all=streamed,
               streamed_over_floor_s=min(streamed) - floor, streamed_over_floor=min(streamed) / floor, timeline=timeline)
    for release in releases:
        release()
    mesh.close()
    ctx.synth_views_free(views)
    g.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

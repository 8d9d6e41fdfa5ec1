"""Measures writing and reading the layers and cameras GeoTIFFs at L = 2 on three routes - the device
(CUDA tensors in, CUDA tensors out), the host loops of liboc_host.so on the threads OpenMP is given, and one thread of zlib
level 6 with numpy's predictor - and writes profiles/layer_files_probe.json.

    python scripts/probe_layer_files.py [--mpx 1 16 256] [--mosaic NX NY] [--repeats 3] [--out profiles/layer_files_probe.json]

--mosaic NX NY: also the "solve" mosaic of probe_ortho_stream_files.py's geometry (synth.make_grid(NX, NY); 40 25 is C3's
1 000 views) with and without the two files, resident and streamed from JPEG files, the two alternating; the files are
io.BytesIO objects, so no disk is in the figures.

Every timing is a host clock around work that ends in a device synchronise (finish / read wait for the context's stream);
the first repeat of every shape is a warm-up and is not counted (one thread of zlib above 16 Mpx runs once, without one); the
median and the spread of the rest are recorded.  The files of all routes hold the same raster: the device's and the host's
are compared byte for byte, zlib's by reading it back.  The mosaic part also splits the time the files cost: a single sweep
with the files against one without is the writer's share, the second sweep's band reads alone are the reader's.
A run measures what its arguments name and keeps the other entries of an --out file that exists, so that the sizes and the
mosaic may come from runs of their own.  A measurement without a device fails: nothing here falls back."""
import argparse
import io
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TILE, L = 512, 2
IDS = np.array([0x0000000100000000, 0x9E3779B97F4A7C15, 0x00000000DEADBEEF, 0x000000000000002A], np.uint64)


def rasters(side):
    """the layered pattern of the tests at side x side: a ragged valid region per layer, smooth colour, four ids"""
    y, x = np.mgrid[0:side, 0:side].astype(np.float32)
    bgra, ids = np.zeros((L, side, side, 4), np.uint8), np.zeros((L, side, side), np.uint64)
    for l in range(L):
        dx, dy = (x - side * (0.45 + 0.1 * l)) / (0.48 * side), (y - side * (0.5 - 0.07 * l)) / (0.46 * side)
        valid = dx * dx + dy * dy < 1.0 + 0.12 * np.sin(7 * np.arctan2(dy, dx) + l)
        colour = np.stack([96 + 80 * np.sin(x / 97.0 + l), 128 + 100 * np.cos(y / 131.0), 60 + (0.1 * (x + y)) % 190,
                           np.full((side, side), 255.0, np.float32)], -1).astype(np.uint8)
        bgra[l][valid] = colour[valid]
        which = ((2 * x // side).astype(np.int64) + 2 * (2 * y // side).astype(np.int64) + l) % 4
        ids[l][valid] = IDS[which][valid]
    return bgra, ids


def interleaved(raster):
    if raster.dtype == np.uint8:
        return np.ascontiguousarray(raster.transpose(1, 2, 0, 3)).reshape(raster.shape[1], raster.shape[2], 4 * L)
    words = raster.view("<u4").reshape(L, raster.shape[1], raster.shape[2], 2)
    return np.ascontiguousarray(words.transpose(1, 2, 0, 3)).reshape(raster.shape[1], raster.shape[2], 2 * L)


def zlib_write(raster):
    """one thread: numpy's predictor and zlib level 6 on every tile that is not all zero; the streams"""
    s = interleaved(raster)
    h, w, n = s.shape
    out = []
    for ty in range(-(-h // TILE)):
        for tx in range(-(-w // TILE)):
            t = np.zeros((TILE, TILE, n), s.dtype)
            part = s[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE]
            t[:part.shape[0], :part.shape[1]] = part
            if not t.any():
                out.append(b"")
                continue
            p = t.copy()
            p[:, 1:] = t[:, 1:] - t[:, :-1]
            out.append(zlib.compress(p.tobytes(), 6))
    return out


def zlib_read(streams, like):
    s_dtype, n = (np.uint8, 4 * L) if like.dtype == np.uint8 else (np.dtype("<u4"), 2 * L)
    h, w = like.shape[1], like.shape[2]
    tw = -(-w // TILE)
    full = np.zeros((-(-h // TILE) * TILE, tw * TILE, n), s_dtype)
    for k, z in enumerate(streams):
        if z:
            ty, tx = divmod(k, tw)
            full[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE] = np.cumsum(
                np.frombuffer(zlib.decompress(z), s_dtype).reshape(TILE, TILE, n), axis=1, dtype=s_dtype)
    s = full[:h, :w]
    if like.dtype == np.uint8:
        return np.ascontiguousarray(s.reshape(h, w, L, 4).transpose(2, 0, 1, 3))
    return np.ascontiguousarray(s.reshape(h, w, L, 2).transpose(2, 0, 1, 3)).view("<u8").reshape(L, h, w)


def timed(fn, repeats, warm=True):
    """(median seconds, min, max, the last result) of fn over `repeats` runs behind one warm-up"""
    if warm:
        fn()
    times, result = [], None
    for _ in range(repeats):
        t = time.perf_counter()
        result = fn()
        times.append(time.perf_counter() - t)
    return dict(median_s=statistics.median(times), min_s=min(times), max_s=max(times)), result


def mosaic(ctx, nx, ny, repeats):
    """the "solve" mosaic without and with the files, resident and streamed from JPEG files: seconds and equality"""
    import torch

    from opencalibration_amd import host, pipeline, synth

    grid = synth.make_grid(nx, ny, feats=16)
    pos = np.ascontiguousarray(grid.position, np.float64)
    n = len(pos)
    rng = np.random.default_rng(0)
    surface = host.rebuild_mesh(pos)
    v = surface.arrays()["vertices"]
    surface.set_heights(v[:, 2] - grid.meta.get("height", 100.0) + rng.uniform(-2, 2, len(v)))
    g = host.Graph()
    m = g.add_model(np.asarray(grid.model, np.float64))
    for p in pos:
        g.add_image(np.zeros((0, 2)), np.zeros(0, np.float32), np.zeros((0, 8), np.uint64), 0, m, p)
    g.set_orientations(np.ascontiguousarray(grid.orientation, np.float64))
    W_img, H_img = int(grid.model[8]), int(grid.model[9])
    plan = host.dsm_plan(g, [surface])
    mesh = host.OrthoMesh(ctx, [surface])
    used = host.ortho_band_cameras(plan, g, [surface], ctx=ctx)
    sets = [set(np.nonzero(row)[0].tolist()) for row in used]
    capacity = max([len(a | b) for a, b in zip(sets, sets[1:])] + [len(s) for s in sets])
    views, _ = pipeline.synthetic_views(ctx, grid)
    files, images = [], []
    one = np.empty((H_img, W_img, 3), np.uint8)
    for i in range(n):
        ctx.synth_views_read_into(views, i, W_img, H_img, one)
        files.append(host.encode_jpeg(np.ascontiguousarray(one[..., ::-1]), ctx=ctx))
    ctx.synth_views_free(views)
    with host.JpegDecoder(ctx) as dec:  # the resident images are the files' pixels: both forms render the same
        for i in range(n):
            images.append(dec.decode([files[i]]).image(0).clone())
    torch.cuda.synchronize()
    raster = torch.empty((plan["height"], plan["width"], 4), dtype=torch.uint8, device="cuda:0")

    def run(form, with_files):
        kw = dict(layers_geotiff=io.BytesIO(), cameras_geotiff=io.BytesIO()) if with_files else {}
        t = time.perf_counter()
        if form == "resident":
            host.ortho_mosaic(plan, g, [surface], images, mesh=mesh, color_balance="solve", out=raster, **kw)
        else:
            host.ortho_mosaic_streamed(plan, g, [surface], None, mesh, capacity, color_balance="solve", out=raster, files=files, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        return dt, (sum(len(f.getvalue()) for f in kw.values()) if with_files else 0)

    out = dict(views=[nx, ny], images=n, width=plan["width"], height=plan["height"], bands=len(sets), capacity=capacity)
    for form in ("resident", "streamed_from_jpeg_files"):
        run(form, False), run(form, True)  # warm-up of both
        want, times, file_bytes = None, {False: [], True: []}, 0
        for _ in range(repeats):  # alternating
            for with_files in (False, True):
                dt, nbytes = run(form, with_files)
                times[with_files].append(dt)
                file_bytes = max(file_bytes, nbytes)
                if want is None:
                    want = raster.clone()
                assert torch.equal(raster, want), "the mosaic with the files is the one without"
        print(f"mosaic: {form} done", file=sys.stderr, flush=True)
        out[form] = dict(without_files_s=statistics.median(times[False]), with_files_s=statistics.median(times[True]),
                         without_all=times[False], with_all=times[True], file_bytes=file_bytes)

    # where the time with the files goes, images resident: the writer's share is a single sweep (no solve, nothing read back)
    # with the files against one without; the reader's share is the second sweep's band reads alone
    kept = {}

    def sweep(with_files):
        kw = dict(layers_geotiff=io.BytesIO(), cameras_geotiff=io.BytesIO()) if with_files else {}
        host.ortho_mosaic(plan, g, [surface], images, mesh=mesh, out=raster, **kw)
        torch.cuda.synchronize()
        kept.update(kw)

    band_rows = host.BLEND_CONFIG["tile_size"]

    def read_bands():
        with host.GeoTiffReader(kept["layers_geotiff"], ctx=ctx) as rl, host.GeoTiffReader(kept["cameras_geotiff"], ctx=ctx) as rc:
            for row0 in range(0, plan["height"], band_rows):
                rows = min(band_rows, plan["height"] - row0)
                rl.read(row0, rows, on_device=True), rc.read(row0, rows, on_device=True)
            torch.cuda.synchronize()

    t_plain, _ = timed(lambda: sweep(False), repeats)
    t_write, _ = timed(lambda: sweep(True), repeats)
    t_read, _ = timed(read_bands, repeats)
    out["split_resident"] = dict(single_sweep_without_files=t_plain, single_sweep_with_files=t_write, second_sweep_band_reads=t_read)
    mesh.close()
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mosaic", type=int, nargs=2, default=None)
    ap.add_argument("--mpx", type=int, nargs="*", default=[1, 16, 256])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layer_files_probe.json"))
    args = ap.parse_args()
    import torch

    torch.cuda.init()
    from opencalibration_amd import capi, host

    ctx = capi.Context(0)
    res = dict(sizes=[])
    if os.path.exists(args.out):  # entries of earlier runs that this one does not measure stay
        with open(args.out) as f:
            res = json.load(f)
    res.update(device=ctx.device_info()["name"], host_threads=int(os.environ.get("OMP_NUM_THREADS", os.cpu_count())), layers=L)
    res.pop("repeats", None)
    for mpx in args.mpx:
        side = int(round((mpx * 1e6) ** 0.5 / 16)) * 16
        bgra, ids = rasters(side)
        d_bgra = torch.from_numpy(bgra).to("cuda:0")
        d_ids = torch.from_numpy(ids.view(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        raw = bgra.nbytes + ids.nbytes

        def write(c, a, b, on_device):
            files = []
            for kind, r in ((host.GEOTIFF_LAYERS8, a), (host.GEOTIFF_CAMERAS32, b)):
                f = io.BytesIO()
                with host.GeoTiffWriter(f, kind, side, side, num_layers=L, ctx=c, on_device=on_device) as wr:
                    for r0 in range(0, side, 1024):  # bands of two tile rows, as a mosaic would feed them
                        wr.feed(r0, r[:, r0:r0 + 1024].contiguous() if on_device else r[:, r0:r0 + 1024])
                    wr.finish()
                files.append(f.getvalue())
            return files

        entry = dict(mpx=mpx, side=side, raw_bytes=raw, repeats=args.repeats)
        print(f"{mpx} Mpx: the rasters are made", file=sys.stderr, flush=True)
        t_dev, f_dev = timed(lambda: write(ctx, d_bgra, d_ids, True), args.repeats)
        t_host, f_host = timed(lambda: write(None, bgra, ids, False), args.repeats)
        assert f_dev == f_host, "the device's files are the host route's"
        print(f"{mpx} Mpx: written by the device and the host loops", file=sys.stderr, flush=True)
        t_zlib, z = timed(lambda: (zlib_write(bgra), zlib_write(ids)), 1 if mpx > 16 else args.repeats, warm=mpx <= 16)
        entry["write"] = dict(device=t_dev, host=t_host, zlib6_one_thread=t_zlib, file_bytes=sum(map(len, f_host)),
                              zlib6_bytes=sum(len(s) for part in z for s in part))

        def read_dev():
            band = host.read_layer_files(f_host[0], f_host[1], ctx=ctx, on_device=True)
            torch.cuda.synchronize()
            return band

        print(f"{mpx} Mpx: written by zlib", file=sys.stderr, flush=True)
        r_dev, band = timed(read_dev, args.repeats)
        assert torch.equal(band["bgra"], d_bgra) and torch.equal(band["camera_id"], d_ids)
        r_host, band = timed(lambda: host.read_layer_files(f_host[0], f_host[1]), args.repeats)
        assert np.array_equal(band["bgra"], bgra) and np.array_equal(band["camera_id"], ids)
        r_zlib, back = timed(lambda: (zlib_read(z[0], bgra), zlib_read(z[1], ids)), 1 if mpx > 16 else args.repeats, warm=mpx <= 16)
        assert np.array_equal(back[0], bgra) and np.array_equal(back[1], ids)
        entry["read"] = dict(device=r_dev, host=r_host, zlib6_one_thread=r_zlib)
        res["sizes"] = sorted([e for e in res["sizes"] if e["mpx"] != mpx] + [entry], key=lambda e: e["mpx"])
        print(json.dumps(entry), flush=True)
        del d_bgra, d_ids, band, back
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:  # after every size: a later one that runs out of time loses nothing
            json.dump(res, f, indent=1)
    if args.mosaic:
        key = f"{args.mosaic[0]}x{args.mosaic[1]}"  # one entry per geometry, each with its own repeats
        res.setdefault("solve_mosaic", {})[key] = dict(mosaic(ctx, args.mosaic[0], args.mosaic[1], args.repeats), repeats=args.repeats)
        print(json.dumps(res["solve_mosaic"][key]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

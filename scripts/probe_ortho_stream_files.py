"""The streamed orthomosaic fed from JPEG files on probe_ortho_stream.py's C3 geometry: the views of
synth.make_grid(NX, NY) rendered on the device, written as baseline JPEG files by the project's encoder and kept in host
memory, then host.ortho_mosaic_streamed three ways in one process, best of --repeats (3), for one sweep (color_balance=None)
and for "solve" (two sweeps):
  (a) files=            the files decoded into the slots on the device (OrthoStream.upload_jpegs);
  (b) fetch, decoded    fetch returns the same pixels decoded beforehand into page-locked memory: the floor without any
                        decode, what the code could already do;
  (c) fetch, host       fetch decodes the file on the host when it is asked: host.decode_jpeg(ctx=None), and Pillow
                        (libjpeg-turbo) where it is importable: what a user does today.
The mosaics of the three ways are checked equal.  Then one layer sweep through OrthoStream itself fed by upload_jpegs,
with the time of the decode calls and of the render per band and the file bytes against the pixel bytes.  Prints one JSON
line and writes it to profiles/ortho_stream_files_probe.json.  --views NX NY (default 40 25, C3's 1 000 views: (c) then
decodes 9 000 images on the host), --capacity N (default: the largest union of two neighbouring bands' sets), --repeats N,
--no-host: leave (c) out.  Needs the GPU."""
import io
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


def note(text):
    print(f"# {text}", file=sys.stderr, flush=True)


def main():
    import torch

    torch.cuda.init()  # torch's HIP runtime comes up before libochip.so is loaded (as in bench.py)
    nx, ny = option("--views", 2, [40, 25])
    repeats, = option("--repeats", 1, [3])
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
    ctx = capi.Context(0)
    W_img, H_img = int(grid.model[8]), int(grid.model[9])
    image_bytes = W_img * H_img * 3
    plan = host.dsm_plan(g, [surface])
    mesh = host.OrthoMesh(ctx, [surface])
    assert len(host.ortho_layers_cameras(g, [surface])["node_ids"]) == n
    used = host.ortho_band_cameras(plan, g, [surface], ctx=ctx)
    sets = [set(np.nonzero(row)[0].tolist()) for row in used]
    capacity, = option("--capacity", 1, [max([len(a | b) for a, b in zip(sets, sets[1:])] + [len(s) for s in sets])])
    out = dict(images=n, image_size=[W_img, H_img], device=ctx.device_info()["name"], width=plan["width"], height=plan["height"],
               bands=len(sets), capacity=capacity, repeats=repeats, set_size_max=max(len(s) for s in sets))

    # the views: rendered on the device, read back, written as JPEG files by the project's encoder (device route), and the
    # files decoded once into page-locked memory for (b)
    views, _ = pipeline.synthetic_views(ctx, grid)
    pixels, release = ctx.host_array((n, H_img, W_img, 3))
    files = []
    t0 = time.perf_counter()
    for i in range(n):
        ctx.synth_views_read_into(views, i, W_img, H_img, pixels[i])
        files.append(host.encode_jpeg(np.ascontiguousarray(pixels[i][..., ::-1]), ctx=ctx))
    ctx.synth_views_free(views)
    with host.JpegDecoder(ctx) as dec:
        for i in range(n):
            pixels[i] = dec.decode([files[i]]).image(0).cpu().numpy()
    out.update(prepare_s=time.perf_counter() - t0, file_bytes=sum(len(f) for f in files), pixel_bytes=n * image_bytes)
    note(f"{n} files of {out['file_bytes'] / n / 1e6:.2f} MB for {image_bytes / 1e6:.1f} MB of pixels each, capacity {capacity}")

    def pillow(i):
        from PIL import Image

        return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(files[i])).convert("RGB"))[..., ::-1])

    ways = {"a_files": dict(fetch=None, files=files), "b_fetch_decoded_page_locked": dict(fetch=lambda i: pixels[i])}
    if "--no-host" not in sys.argv:
        ways["c_fetch_host_loops"] = dict(fetch=lambda i: host.decode_jpeg(files[i]))
        try:
            import PIL  # noqa: F401

            ways["c_fetch_pillow"] = dict(fetch=pillow)
        except ImportError:
            pass
    raster = torch.empty((plan["height"], plan["width"], 4), dtype=torch.uint8, device="cuda:0")
    want = {}
    for balance in (None, "solve"):
        key = "solve" if balance else "one_sweep"
        out[key] = {}
        for name, how in ways.items():
            times = []
            for r in range(repeats + (name == "a_files")):  # the first way's first run warms the pools up and is dropped
                t0 = time.perf_counter()
                host.ortho_mosaic_streamed(plan, g, [surface], how["fetch"], mesh, capacity, color_balance=balance, out=raster,
                                           files=how.get("files"))
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            if name == "a_files":
                times = times[1:]
                want[key] = raster.clone()
            out[key][name] = dict(s=min(times), s_all=times, equal_to_a=bool(torch.equal(raster, want[key])))
            note(f"{key} {name}: {min(times):.3f} s")
        a, b = out[key]["a_files"]["s"], out[key]["b_fetch_decoded_page_locked"]["s"]
        out[key]["a_over_b"] = a / b
        out[key]["a_minus_b_s"] = a - b
        for name in ways:
            if name.startswith("c_"):
                out[key][name + "_over_a"] = out[key][name]["s"] / a

    # one layer sweep through the stream itself: the decode calls and the render per band
    cfg = host.LAYERS_CONFIG
    T, L, W, H = cfg["tile_size"], cfg["num_layers"], plan["width"], plan["height"]
    bufs = dict(bgra=torch.empty((L, T, W, 4), dtype=torch.uint8, device="cuda:0"),
                camera_id=torch.empty((L, T, W), dtype=torch.int64, device="cuda:0"))

    def band_out(rows):
        return {k: t.view(-1)[:t[:, :rows].numel()].view(t[:, :rows].shape) for k, t in bufs.items()}

    best = None
    for _ in range(repeats):
        rows = []
        with host.OrthoStream(plan, g, [surface], capacity, mesh=mesh, tile_rows=1) as stream:
            t_start = time.perf_counter()
            for k in range(stream.num_bands):
                row = dict(band=k, cameras=len(stream.band_cameras(k)), files=0, file_bytes=0, pixel_bytes=0, decode_ms=0.0)
                calls = [(k, stream.loads(k) if k == 0 else stream.loads(k, host.LOAD_LATE))]
                if k + 1 < stream.num_bands:
                    calls.append((k + 1, stream.loads(k + 1, host.LOAD_AHEAD)))
                for b, loads in calls:
                    cams = [cam for cam, _, _ in loads]
                    if cams:
                        t0 = time.perf_counter()
                        stream.upload_jpegs(b, cams, [files[c] for c in cams])
                        row["decode_ms"] += (time.perf_counter() - t0) * 1e3
                        row["files"] += len(cams)
                        row["file_bytes"] += sum(len(files[c]) for c in cams)
                        row["pixel_bytes"] += len(cams) * image_bytes
                t0 = time.perf_counter()
                stream.render(k, out=band_out(min(T, H - k * T)))
                row["render_ms"] = (time.perf_counter() - t0) * 1e3
                rows.append(row)
            total = time.perf_counter() - t_start
        if best is None or total < best[0]:
            best = (total, rows)
    out.update(layer_sweep_s=best[0], layer_sweep_decode_s=sum(r["decode_ms"] for r in best[1]) / 1e3,
               layer_sweep_render_s=sum(r["render_ms"] for r in best[1]) / 1e3,
               decode_ms_per_file=sum(r["decode_ms"] for r in best[1]) / max(1, sum(r["files"] for r in best[1])), per_band=best[1])
    release()
    mesh.close()
    g.close()
    ctx.close()
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "ortho_stream_files_probe.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

"""The JPEG texture at 1, 16 and 256 Mpx of a ramp-plus-noise raster: the device route from a device
tensor and from host memory, the CPU route on the threads OpenMP has, and Pillow (libjpeg-turbo on one thread, the shape of
the reference's cv::imwrite), alternating in one process, three runs each (at 256 Mpx the two CPU encoders run once), every
result checked equal, best of three.  Prints one JSON line per size.  --c3: also the C3-geometry mosaic of
probe_ortho_blend.py - ortho_mosaic without and with jpeg=, alternating, three runs each, and encode_jpeg of the finished
mosaic from the device tensor.  --quick: one encode of 16 Mpx from a device tensor (the kernel-trace run).  Needs the GPU."""
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opencalibration_amd import capi, host, pipeline, synth  # noqa: E402


def raster(side, seed=0):
    """ramp plus noise of amplitude 16, RGBA"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:side, 0:side].astype(np.uint16)
    out = np.empty((side, side, 4), np.uint8)
    for c, (a, b) in enumerate(((5, 3), (2, 7), (1, 1))):
        out[..., c] = ((a * x + b * y) // 8 + rng.integers(0, 16, (side, side), dtype=np.uint16)) % 256
    out[..., 3] = 255
    return out


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    res = fn()
    sync()
    return time.perf_counter() - t0, res


def pillow_bytes(rgb):
    from PIL import Image

    f = io.BytesIO()
    Image.fromarray(rgb).save(f, format="JPEG", quality=95)
    return f.getvalue()


def main():
    import torch

    torch.cuda.init()  # torch's HIP runtime comes up before libochip.so is loaded (as in bench.py)
    quick, c3 = "--quick" in sys.argv, "--c3" in sys.argv
    ctx = capi.Context(0)
    sync = torch.cuda.synchronize
    try:
        import PIL  # noqa: F401
        have_pillow = True
    except ImportError:
        have_pillow = False
    for side in ((4096,) if quick else (1024, 4096, 16384)):
        rgba = raster(side)
        rgb = np.ascontiguousarray(rgba[..., :3])
        d = torch.from_numpy(rgba).to("cuda:0")
        sync()
        line = dict(device=ctx.device_info()["name"], side=side, mpx=side * side / 1e6, cpu_threads=os.environ.get("OMP_NUM_THREADS"))
        if quick:
            line["device_tensor_s"] = timed(lambda: host.encode_jpeg(d, ctx=ctx), sync)[0]
            print(json.dumps(line))
            continue
        want = host.encode_jpeg(d, ctx=ctx)  # warms the pools
        runs = 3
        cpu_runs = 1 if side > 8192 else 3
        t = dict(device_tensor=[], device_from_host=[], cpu_route=[], pillow=[])
        equal = True
        for k in range(runs):
            s, got = timed(lambda: host.encode_jpeg(d, ctx=ctx), sync)
            t["device_tensor"].append(s), (equal := equal and got == want)
            s, got = timed(lambda: host.encode_jpeg(rgb, ctx=ctx), sync)
            t["device_from_host"].append(s), (equal := equal and got == want)
            if k < cpu_runs:
                s, got = timed(lambda: host.encode_jpeg(rgb), sync)
                t["cpu_route"].append(s), (equal := equal and got == want)
                if have_pillow:
                    s, got = timed(lambda: pillow_bytes(rgb), sync)
                    t["pillow"].append(s), (equal := equal and got == want)
        line.update(file_bytes=len(want), bits_per_pixel=8 * len(want) / side / side, all_equal=equal)
        for k, v in t.items():
            if v:
                line[k + "_s_all"] = v
                line[k + "_s"] = min(v)
                line[k + "_mpx_per_s"] = side * side / 1e6 / min(v)
        print(json.dumps(line), flush=True)
        del d
    if c3:
        grid = synth.make_grid(40, 25, feats=16)
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
        W_img, H_img = int(grid.model[8]), int(grid.model[9])
        views, _ = pipeline.synthetic_views(ctx, grid)
        ptrs = [int(views) + i * W_img * H_img * 3 for i in range(len(pos))]
        plan = host.dsm_plan(g, [surface])
        W, H = plan["width"], plan["height"]
        mesh = host.OrthoMesh(ctx, [surface])
        mosaic = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")

        def end_to_end(jpeg):
            f = io.BytesIO() if jpeg else None
            s, _ = timed(lambda: host.ortho_mosaic(plan, g, [surface], ptrs, mesh=mesh, out=mosaic, jpeg=f), sync)
            return s, (f.getvalue() if jpeg else None)

        end_to_end(True)  # warms the pools and the allocator for both
        plain, with_jpeg, data = [], [], None
        for _ in range(3):
            plain.append(end_to_end(False)[0])
            s, data = end_to_end(True)
            with_jpeg.append(s)
        alone = [timed(lambda: host.encode_jpeg(mosaic, ctx=ctx), sync) for _ in range(3)]
        line = dict(c3=True, width=W, height=H, gpx=W * H / 1e9, mosaic_s_all=plain, mosaic_jpeg_s_all=with_jpeg, mosaic_s=min(plain),
                    mosaic_jpeg_s=min(with_jpeg), yardstick_spread=(max(plain) - min(plain)) / min(plain),
                    jpeg_excess=min(with_jpeg) / min(plain) - 1.0, encode_alone_s_all=[a[0] for a in alone],
                    encode_alone_s=min(a[0] for a in alone), file_bytes=len(data), files_equal=all(a[1] == data for a in alone),
                    opaque_fraction=float((mosaic[..., 3] == 255).float().mean().item()))
        print(json.dumps(line), flush=True)
        mesh.close()
        ctx.synth_views_free(views)
        g.close()
    ctx.close()


if __name__ == "__main__":
    main()

"""The tiled DEFLATE GeoTIFF writer at 1, 16 and 256 Mpx of a ramp-plus-noise RGBA raster, without overview
levels: the device route from a device tensor, the CPU route on the threads OpenMP has, and zlib.compress(level=6) of the same
predicted tile payloads on one thread - the work of the reference's GDAL call - alternating in one process, three runs each
(at 256 Mpx the two CPU encoders run once), the two routes' files checked equal, best of three.  The files go to a sink that
counts and discards - and digests, in one run per route ahead of the timed ones - so no disk is timed; the file's bytes are what crosses PCIe on the device route.  Prints one
JSON line per size.  --c3: also the C3-geometry mosaic of probe_ortho_blend.py - ortho_mosaic without and with geotiff= and dsm_geotiff=,
alternating, three runs each, the sinks' digests taken in two runs ahead of the timed ones.  --quick: one 16 Mpx file from a device tensor (the kernel-trace run).  Needs the GPU."""
import hashlib
import io
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opencalibration_amd import capi, host, pipeline, synth  # noqa: E402


class Sink(io.RawIOBase):
    """a seekable binary target that keeps a digest of what is written in order, and the length"""

    def __init__(self, check=True):
        super().__init__()
        self.at = self.size = 0
        self.digest = hashlib.blake2b(digest_size=16) if check else None

    def seekable(self):
        return True

    def writable(self):
        return True

    def tell(self):
        return self.at

    def seek(self, at, whence=0):
        self.at = at if whence == 0 else self.at + at if whence == 1 else self.size + at
        return self.at

    def write(self, data):
        n = len(data)
        if self.digest is not None:
            self.digest.update(self.at.to_bytes(8, "little"))
            self.digest.update(data)
        self.at += n
        self.size = max(self.size, self.at)
        return n


def raster(side, seed=0):
    """ramp plus noise of amplitude 4, RGBA, a transparent border of a sixteenth"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:side, 0:side].astype(np.uint16)
    out = np.empty((side, side, 4), np.uint8)
    for c, (a, b) in enumerate(((5, 3), (2, 7), (1, 1))):
        out[..., c] = ((a * x + b * y) // 8 + rng.integers(0, 4, (side, side), dtype=np.uint16)) % 256
    out[..., 3] = 255
    e = side // 16
    out[:e], out[-e:], out[:, :e], out[:, -e:] = 0, 0, 0, 0
    return out


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    res = fn()
    sync()
    return time.perf_counter() - t0, res


def write(r, ctx, check=False):
    """the file's size, and with check its digest (about a second per GB: outside the timed runs)"""
    s = Sink(check)
    host.save_geotiff(s, r, ctx=ctx, overviews=False)
    return (s.size, s.digest.hexdigest()) if check else s.size


def zlib6(rgba):
    """seconds and bytes of zlib level 6 over the predicted payloads of the raster's tiles, one thread; the predictor is not timed"""
    side, secs, size = rgba.shape[0], 0.0, 0
    for ty in range(0, side, 512):
        for tx in range(0, side, 512):
            t = np.zeros((512, 512, 4), np.uint8)
            part = rgba[ty:ty + 512, tx:tx + 512]
            t[:part.shape[0], :part.shape[1]] = part
            p = t.copy()
            p[:, 1:] = t[:, 1:] - t[:, :-1]
            data = p.tobytes()
            t0 = time.perf_counter()
            size += len(zlib.compress(data, 6))
            secs += time.perf_counter() - t0
    return secs, size


def main():
    import torch

    torch.cuda.init()  # torch's HIP runtime comes up before libochip.so is loaded (as in bench.py)
    quick, c3 = "--quick" in sys.argv, "--c3" in sys.argv
    ctx = capi.Context(0)
    sync = torch.cuda.synchronize
    for side in ((4096,) if quick else (1024, 4096, 16384)):
        rgba = raster(side)
        d = torch.from_numpy(rgba).to("cuda:0")
        sync()
        line = dict(device=ctx.device_info()["name"], side=side, mpx=side * side / 1e6, cpu_threads=os.environ.get("OMP_NUM_THREADS"))
        if quick:
            write(d, ctx)
            line["device_tensor_s"] = timed(lambda: write(d, ctx), sync)[0]
            print(json.dumps(line))
            continue
        want = write(d, ctx, True)  # warms the pools
        cpu_runs = 1 if side > 8192 else 3
        t = dict(device_tensor=[], cpu_route=[], zlib6=[])
        equal, z6 = write(rgba, None, True) == want, 0
        for k in range(3):
            s, got = timed(lambda: write(d, ctx), sync)
            t["device_tensor"].append(s), (equal := equal and got == want[0])
            if k < cpu_runs:
                s, got = timed(lambda: write(rgba, None), sync)
                t["cpu_route"].append(s), (equal := equal and got == want[0])
                s, z6 = zlib6(rgba)
                t["zlib6"].append(s)
        line.update(file_bytes=want[0], raster_bytes=rgba.nbytes, zlib6_bytes=z6, size_over_zlib6=want[0] / z6, routes_equal=equal)
        for k, v in t.items():
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

        def end_to_end(tiff, over=False, check=False):
            a, b = (Sink(check), Sink(check)) if tiff else (None, None)
            s, _ = timed(lambda: host.ortho_mosaic(plan, g, [surface], ptrs, mesh=mesh, out=mosaic, geotiff=a, dsm_geotiff=b,
                                                   overviews=over), sync)
            return s, ((a.size, b.size) + ((a.digest.hexdigest(), b.digest.hexdigest()) if check else ()) if tiff else None)

        data = [end_to_end(True, check=True)[1] for _ in range(2)]  # warms the pools and the allocator; the digests are not timed
        plain, with_over, with_tiff = [], [], []
        for _ in range(3):
            plain.append(end_to_end(False)[0])
            with_over.append(end_to_end(False, True)[0])
            s, got = end_to_end(True)
            with_tiff.append(s), data.append(got + data[0][2:])
        line = dict(c3=True, width=W, height=H, gpx=W * H / 1e9, mosaic_s_all=plain, mosaic_overviews_s_all=with_over,
                    mosaic_geotiff_s_all=with_tiff, mosaic_s=min(plain), mosaic_overviews_s=min(with_over), mosaic_geotiff_s=min(with_tiff),
                    yardstick_spread=(max(plain) - min(plain)) / min(plain), orthomosaic_bytes=data[0][0], dsm_bytes=data[0][1],
                    raster_bytes=W * H * 4, files_equal=all(x == data[0] for x in data))
        print(json.dumps(line), flush=True)
        mesh.close()
        ctx.synth_views_free(views)
        g.close()
    ctx.close()


if __name__ == "__main__":
    main()

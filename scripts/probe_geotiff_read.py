"""The tiled DEFLATE GeoTIFF reader from a file in host memory to the raster: a 16 384 x 16 384 RGBA mosaic
(1 024 tiles) and a DSM of the same size, and a 4 096 x 4 096 mosaic (64 tiles) to show where the routes cross.  Two files
per raster: written by this project's writer, and the same pixels through the tests' builder at zlib level 6.  Three routes:
the device route into a device tensor, the host route on the threads OpenMP has, and zlib.decompress plus numpy on one thread -
alternating in one process, best of three (the single thread runs once at 1 024 tiles), every result checked equal to the
raster.  Prints one JSON line per file.  --quick: one device read of the 1 024-tile mosaic (the kernel-trace run).  Needs the
GPU."""
import io
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

import geotiff_read_fixtures as R  # noqa: E402
from probe_geotiff import raster, timed  # noqa: E402
from opencalibration_amd import capi, host  # noqa: E402


def surface(side, seed=0):
    """a smooth float32 surface with noise of a millimetre and NaN outside a border of a sixteenth"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:side, 0:side].astype(np.float32)
    d = (100 + 0.01 * x + 0.02 * y + np.sin(x / 370) * np.cos(y / 230)).astype(np.float32)
    d += rng.normal(0, 0.001, d.shape).astype(np.float32)
    e = side // 16
    d[:e], d[-e:], d[:, :e], d[:, -e:] = np.nan, np.nan, np.nan, np.nan
    return d


def single_thread(data, out):
    """zlib.decompress and numpy over the tiles of the file's first IFD, into out"""
    with host.GeoTiffReader(data) as rd:
        lv = rd._ifds[0]
        tw, th, w, h = lv["tile_w"], lv["tile_h"], lv["width"], lv["height"]
        for i, (o, c) in enumerate(zip(lv["offsets"], lv["counts"])):
            ty, tx = divmod(i, lv["tiles_x"])
            rows, cols = min(th, h - ty * th), min(tw, w - tx * tw)
            if c == 0:
                out[ty * th:ty * th + rows, tx * tw:tx * tw + cols] = 0
                continue
            raw = zlib.decompress(rd.buf[int(o):int(o + c)])
            if lv["is_float"]:
                t = np.cumsum(np.frombuffer(raw, np.uint32).reshape(th, tw), axis=1, dtype=np.uint32).view(np.float32)
            else:
                t = np.cumsum(np.frombuffer(raw, np.uint8).reshape(th, tw, -1), axis=1, dtype=np.uint8)
            out[ty * th:ty * th + rows, tx * tw:tx * tw + cols] = t[:rows, :cols]
    return out


def main():
    import torch

    torch.cuda.init()  # torch's HIP runtime comes up before libochip.so is loaded (as in bench.py)
    quick = "--quick" in sys.argv
    ctx = capi.Context(0)
    sync = torch.cuda.synchronize
    cases = [("rgba", 16384)] if quick else [("rgba", 4096), ("rgba", 16384), ("dsm", 16384)]
    for what, side in cases:
        a = raster(side) if what == "rgba" else surface(side)
        d = torch.from_numpy(a).to("cuda:0")
        sync()
        f = io.BytesIO()
        host.save_geotiff(f, d, ctx=ctx, overviews=False)
        files = {"project_writer": f.getvalue()}
        if not quick:
            files["builder_zlib6"] = R.build_tiff(a, level=6, sparse=True, threads=16)
        for variant, data in files.items():
            tiles = (-(-side // 512)) ** 2
            line = dict(device=ctx.device_info()["name"], raster=what, side=side, tiles=tiles, file=variant, file_bytes=len(data),
                        raster_bytes=a.nbytes, cpu_threads=os.environ.get("OMP_NUM_THREADS"))
            out_d = torch.empty_like(d)
            with host.GeoTiffReader(data, ctx=ctx) as dr, host.GeoTiffReader(data) as hr:
                dr.read(out=out_d, on_device=True)  # warms the pools
                if quick:
                    line["device_s"] = timed(lambda: dr.read(out=out_d, on_device=True), sync)[0]
                    print(json.dumps(line), flush=True)
                    continue
                same = lambda t: bool(torch.equal(t.view(torch.int32), d.view(torch.int32)))
                out_h = np.empty_like(a)
                t = dict(device=[], host_route=[], zlib_numpy_one_thread=[])
                equal = same(out_d)
                for k in range(3):
                    out_d.zero_()
                    sync()
                    t["device"].append(timed(lambda: dr.read(out=out_d, on_device=True), sync)[0])
                    equal = equal and same(out_d)
                    t["host_route"].append(timed(lambda: hr.read(out=out_h), sync)[0])
                    equal = equal and out_h.tobytes() == a.tobytes()
                    if k == 0 or tiles <= 64:
                        out_h[...] = 0
                        t["zlib_numpy_one_thread"].append(timed(lambda: single_thread(data, out_h), sync)[0])
                        equal = equal and out_h.tobytes() == a.tobytes()
            line["results_equal"] = equal
            for k, v in t.items():
                line[k + "_s_all"] = v
                line[k + "_s"] = min(v)
                line[k + "_mpx_per_s"] = side * side / 1e6 / min(v)
            print(json.dumps(line), flush=True)
        del d
    ctx.close()


if __name__ == "__main__":
    main()

"""The JPEG decoder at 1, 4 and 20 Mpx in 4:2:0 and 4:2:2 of a ramp-plus-noise picture written by Pillow
at quality 95: the device route in batches (files in host memory to pixels on the device), the host loops on the threads
OpenMP has, and Pillow (libjpeg-turbo on one thread, the shape of the reference's cv::imread), three runs each, every result
checked equal, best of three, microseconds per image - beside the extraction's microseconds per image at the bench's image
size (4000 x 3000 synthetic views through Graph.load_images).  Also the subsequence lengths 256 .. 8192 bits at 20 Mpx
4:2:0 with their rounds.  Prints one JSON line per measurement and writes them to profiles/jpeg_decode_probe.json.
--quick: one batch of four 20 Mpx 4:2:0 files on the device (the kernel-trace run).  Needs the GPU and Pillow."""
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opencalibration_amd import capi, host, pipeline, synth  # noqa: E402

SIZES = {"1 Mpx": (864, 1152, 16), "4 Mpx": (1728, 2304, 8), "20 Mpx": (3888, 5184, 4)}  # height, width, batch


def picture(h, w, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.uint16)
    out = np.empty((h, w, 3), np.uint8)
    for c, (a, b) in enumerate(((5, 3), (2, 7), (1, 1))):
        out[..., c] = ((a * x + b * y) // 8 + rng.integers(0, 16, (h, w), dtype=np.uint16)) % 256
    return out


def pillow_file(rgb, subsampling):
    from PIL import Image

    f = io.BytesIO()
    Image.fromarray(rgb).save(f, format="JPEG", quality=95, subsampling=subsampling)
    return f.getvalue()


def pillow_pixels(data):
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1]


def best(fn, runs=3):
    out, res = [], None
    for _ in range(runs):
        t0 = time.perf_counter()
        res = fn()
        out.append(time.perf_counter() - t0)
    return min(out), res


def main():
    import torch

    torch.cuda.init()  # torch's HIP runtime comes up before libochip.so is loaded (as in bench.py)
    ctx = capi.Context(0)
    lines = []

    def report(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    if "--quick" in sys.argv:
        h, w, batch = SIZES["20 Mpx"]
        files = [pillow_file(picture(h, w, i), 2) for i in range(batch)]
        with host.JpegDecoder(ctx) as d:
            d.decode(files)
            s, b = best(lambda: d.decode(files), 1)
        print(json.dumps(dict(quick=True, us_per_image=s / batch * 1e6, rounds=b.rounds)))
        ctx.close()
        return
    for label, (h, w, batch) in SIZES.items():
        for sampling, sub in (("4:2:0", 2), ("4:2:2", 1)):
            files = [pillow_file(picture(h, w, i), sub) for i in range(batch)]
            with host.JpegDecoder(ctx) as d:
                out = torch.empty(batch * h * w * 3, dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                d.decode(files, out=out)  # warms the pools
                dev_s, b = best(lambda: d.decode(files, out=out))
            with host.JpegDecoder() as d:
                cpu_s, c = best(lambda: d.decode(files))
            pil_s, p = best(lambda: pillow_pixels(files[0]))
            assert b.status == c.status == ["ok"] * batch
            assert np.array_equal(b.pixels.cpu().numpy(), c.pixels) and np.array_equal(c.image(0), p)
            report(dict(size=label, height=h, width=w, sampling=sampling, batch=batch, file_bytes=len(files[0]),
                        device_us_per_image=dev_s / batch * 1e6, host_openmp_us_per_image=cpu_s / batch * 1e6,
                        host_threads=os.cpu_count() if "OMP_NUM_THREADS" not in os.environ else int(os.environ["OMP_NUM_THREADS"]),
                        pillow_one_thread_us_per_image=pil_s * 1e6, rounds=b.rounds))
    h, w, batch = SIZES["20 Mpx"]
    files = [pillow_file(picture(h, w, i), 2) for i in range(batch)]
    for bits in (256, 512, 1024, 2048, 4096, 8192):
        with host.JpegDecoder(ctx, subsequence_bits=bits) as d:
            d.decode(files)
            s, b = best(lambda: d.decode(files))
        report(dict(subsequence_bits=bits, size="20 Mpx", sampling="4:2:0", batch=batch, device_us_per_image=s / batch * 1e6, rounds=b.rounds))
    grid = synth.make_grid(2, 4)
    ptr, (n, gh, gw) = pipeline.synthetic_views(ctx, grid)
    g = host.Graph()
    m = g.add_model(grid.model)
    g.load_images(ctx, ptr, m, grid.position, device_shape=(n, gh, gw))
    ctx.synchronize()
    ext_s, _ = best(lambda: (g.load_images(ctx, ptr, m, grid.position, device_shape=(n, gh, gw)), ctx.synchronize()))
    report(dict(extraction=True, height=gh, width=gw, batch=n, extract_us_per_image=ext_s / n * 1e6))
    g.close()
    ctx.synth_views_free(ptr)
    with open(os.path.join(ROOT, "profiles", "jpeg_decode_probe.json"), "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()

"""Where PNG encoding costs what: batches of 1 000 and 5 000 noisy thumbnails (58 x 43 RGB) and one
1 024^2 and one 4 096^2 RGBA preview through the device route, the host loops and Pillow on one thread at compress_level 1
(the work inside cv::imencode's default: filter Sub, Z_BEST_SPEED, Z_RLE) and at its default.  Best of three, the routes
alternating in one process; the files' sizes beside the times.  No threshold is set here: the numbers are written down.

  python scripts/probe_png.py [--out profiles/png_probe.json] [--only thumbnails | previews]

rocprofv3 --kernel-trace --stats -- python scripts/probe_png.py --only thumbnails   (or previews) shows where the kernel time goes."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from PIL import Image  # noqa: E402

import png_fixtures as F  # noqa: E402
from opencalibration_amd import capi, host  # noqa: E402


def pillow(batch, level):
    total = 0
    for a in batch:
        f = io.BytesIO()
        Image.fromarray(a).save(f, "PNG", **({} if level is None else dict(compress_level=level)))
        total += f.tell()
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_probe.json"))
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    photo = F.image("rgba_photo")
    cases = dict(thumbnails_1000=F.thumb_batch(1000), thumbnails_5000=[a for _ in range(5) for a in F.thumb_batch(1000)])
    if args.only == "previews":
        cases = {}
    if args.only != "thumbnails":
        cases["preview_1024"] = [np.ascontiguousarray(np.tile(photo, (2, 1, 1))[:1024, :1024])]
        cases["preview_4096"] = [np.ascontiguousarray(np.tile(photo, (6, 4, 1))[:4096, :4096])]
    ctx = capi.Context(0)
    dev, cpu = host.PngEncoder(ctx), host.PngEncoder()
    result = dict(device=ctx.device_info()["name"], host_threads=int(os.environ["OMP_NUM_THREADS"]), cases={})
    for name, batch in cases.items():
        tensors = [torch.from_numpy(a).to("cuda:0") for a in batch]
        torch.cuda.synchronize()
        routes = dict(device_numpy=lambda: sum(map(len, dev.encode(batch))), device_tensors=lambda: sum(map(len, dev.encode(tensors))),
                      device_tensors_base64=lambda: sum(map(len, dev.encode(tensors, base64=True))),
                      host_loops=lambda: sum(map(len, cpu.encode(batch))), pillow_level_1=lambda: pillow(batch, 1),
                      pillow_default=lambda: pillow(batch, None))
        dev.encode(batch)  # the encoder's arrays and the first launches
        best, size = {k: float("inf") for k in routes}, {}
        for _ in range(3):
            for k, run in routes.items():
                t0 = time.perf_counter()
                size[k] = run()
                best[k] = min(best[k], time.perf_counter() - t0)
        rec = dict(images=len(batch), pixels=int(sum(a.shape[0] * a.shape[1] for a in batch)),
                   seconds={k: round(v, 6) for k, v in best.items()}, bytes=size)
        rec["device_over_pillow_level_1"] = round(best["pillow_level_1"] / best["device_tensors"], 2)
        rec["device_over_host_loops"] = round(best["host_loops"] / best["device_tensors"], 2)
        result["cases"][name] = rec
        print(name, json.dumps(rec), flush=True)
    dev.close(), cpu.close(), ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

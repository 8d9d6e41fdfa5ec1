"""The load stage's thumbnail pass on C3's views: the 1 000 views of synth.make_grid(40, 25) rendered into HBM
(synth_views), then in one process the one-off fill of the table of all BGR codes, the thumbnail pass over all views
(warm, best of 3, the call returns with the thumbnails on the host), the load stage's extraction on the same views as
the yardstick, and the same pass over random-colour images, the table gather's worst case.  Prints one JSON line; the
pass is stated per image, as a multiple of the floor (the image read once at the HBM rate DESIGN.md §4.8 measured) and
as a fraction of the extraction.  --quick: one pass over 64 views, for a kernel-trace run.  Needs the GPU."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opencalibration_amd import capi, host, pipeline, synth  # noqa: E402

HBM_TBPS = 6.29


def best_of(fn, runs):
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return min(times), times


def main():
    import torch

    torch.cuda.init()  # torch's HIP runtime comes up before libochip.so is loaded (as in bench.py)
    quick = "--quick" in sys.argv
    grid = synth.make_grid(40, 25, feats=16)
    n = 64 if quick else grid.n_images
    ctx = capi.Context(0)
    w, h = int(grid.model[8]), int(grid.model[9])
    views, _ = pipeline.synthetic_views(ctx, grid, block=(0, n))
    shape = (n, h, w)
    out = dict(images=n, image_size=[w, h], thumbnail=list(host.thumbnail_size(w, h)), device=ctx.device_info()["name"])

    t0 = time.perf_counter()
    _, fill_ms = ctx.lab_table([])
    out["table_first_use_s"] = time.perf_counter() - t0  # allocation, fill and wait
    out["table_fill_kernel_ms"] = fill_ms

    thumbs = host.image_thumbnails(views, ctx, device_shape=shape)  # warms the pool
    if not quick:
        t, all_t = best_of(lambda: host.image_thumbnails(views, ctx, device_shape=shape), 3)
        out["thumbnails_s"], out["thumbnails_s_all"] = t, all_t
        out["thumbnail_us_per_image"] = 1e6 * t / n
        floor_us = w * h * 3 / (HBM_TBPS * 1e12) * 1e6
        out["floor_us_per_image"] = floor_us
        out["pass_over_floor"] = out["thumbnail_us_per_image"] / floor_us

        def extract():
            g = host.Graph()
            g.load_images(ctx, views, g.add_model(np.asarray(grid.model, np.float64)), grid.position[:n], device_shape=shape)
            g.close()

        extract()
        t, all_t = best_of(extract, 2)
        out["extract_s"], out["extract_s_all"] = t, all_t
        out["extract_us_per_image"] = 1e6 * t / n
        out["pass_over_extract"] = out["thumbnail_us_per_image"] / out["extract_us_per_image"]

    # the worst case of the gather: every pixel another colour
    n_rand = 16 if quick else 64
    noise = torch.randint(0, 256, (n_rand, h, w, 3), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rshape = (n_rand, h, w)
    rthumbs = host.image_thumbnails(noise.data_ptr(), ctx, device_shape=rshape)
    if not quick:
        t, all_t = best_of(lambda: host.image_thumbnails(noise.data_ptr(), ctx, device_shape=rshape), 3)
        out["random_us_per_image"], out["random_s_all"] = 1e6 * t / n_rand, all_t
        t, _ = best_of(lambda: host.image_thumbnails(views, ctx, device_shape=rshape), 3)
        out["views_same_batch_us_per_image"] = 1e6 * t / n_rand
        # the CPU route on one view and one noise image: the same bytes
        one = ctx.synth_views_read(views, 0, w, h)
        out["cpu_equal_view"] = bool(np.array_equal(host.image_thumbnails(one[None]), thumbs[:1]))
        out["cpu_equal_noise"] = bool(np.array_equal(host.image_thumbnails(noise[:1].cpu().numpy()), rthumbs[:1]))
    out["distinct_thumbnail_values"] = [int(len(np.unique(thumbs))), int(len(np.unique(rthumbs)))]
    del noise
    ctx.synth_views_free(views)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

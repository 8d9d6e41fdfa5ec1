"""The scenarios of test_gpu_ortho_layers_oracle.py, run in a child process for layers_gpu_child.py's reasons (torch brings
up its HIP runtime before libochip.so is loaded; the device route reads its images from torch tensors).
`python layers_oracle_gpu_child.py <tests dir> <repo dir>` renders scenes A - E of layers_oracle_scenes.py on the device,
compares each with the long-double reference fed the device's own kNN lists and DSM band, and prints one JSON line
{scene: {"result": "ok" or the failure's traceback, "seconds": the scenario's wall time, "stats": the reference's counts}}."""
import json
import sys
import time
import traceback

import torch

torch.cuda.init()
if __name__ == "__main__":
    sys.path[:0] = sys.argv[1:3]

from layers_oracle_scenes import SCENES, check_route  # noqa: E402
from opencalibration_amd import capi, host  # noqa: E402


def scenario(ctx, name):
    make, expect = SCENES[name]
    scene = make()
    try:
        images = [torch.from_numpy(im).to("cuda:0") for im in scene.images]
        with host.OrthoMesh(ctx, scene.surfaces) as mesh:
            dev = host.ortho_layers(scene.plan, scene.graph, scene.surfaces, images, mesh=mesh, config=scene.cfg, debug_knn=True)
            dsm = host.dsm_render(scene.plan, scene.surfaces, mesh=mesh)
        return check_route(scene, dev, dsm, expect)
    finally:
        scene.close()


if __name__ == "__main__":
    ctx = capi.Context(0)
    res = {}
    for name in SCENES:
        t0 = time.perf_counter()
        try:
            res[name] = dict(result="ok", stats=scenario(ctx, name))
        except Exception:
            res[name] = dict(result=traceback.format_exc())
        res[name]["seconds"] = round(time.perf_counter() - t0, 3)
    ctx.close()
    print(json.dumps(res))

"""The point cloud file by three routes at 10^3, 10^4, 10^5 points and at the 650 000 points of the
DENSE_MESH_RELAX stand-in (probe_dense_mesh_relax.py's cloud): (a) the device route - upload, box, lines + scan, scatter +
download timed apart -, also from a cloud a MeshPoints object already holds; (b) the host loops under OpenMP (ctx=None);
(c) the yardstick program tests/xyz_export_driver.cpp - std::map and ostream on one thread, the reference's shape.  The
routes alternate in one process, three runs each, every run listed and every result compared.
Usage: probe_xyz_export.py [--out FILE] [--export-only]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

from opencalibration_amd import capi, host
from probe_dense_mesh_relax import scene

SIZES = (1000, 10_000, 100_000, 650_000)


def timed(f):
    t = time.perf_counter()
    r = f()
    return time.perf_counter() - t, r


def device_run(ctx, cloud, points=None):
    """One export on the device, its steps timed apart (each call ends in a wait for the stream)."""
    t = {}
    t["create_s"], e = timed(lambda: capi.XyzExport(ctx, cloud) if points is None else capi.XyzExport.from_points(ctx, points))
    t["bounds_s"], box = timed(e.bounds)
    t["text_size_s"], (nbytes, kept) = timed(lambda: e.text_size(box))
    out = np.zeros(max(nbytes, 1), np.uint8)
    t["text_s"], rc = timed(lambda: e.L.ochip_xyz_export_text(e.h, out.ctypes.data, nbytes))
    assert rc == 0
    e.close()
    t["total_s"] = sum(t.values())
    return t, box, out[:nbytes].tobytes()


def host_run(cloud):
    t = {}
    t["bounds_s"], box = timed(lambda: host.cloud_outlier_bounds(cloud))
    t["text_s"], text = timed(lambda: host.cloud_to_xyz(cloud, bounds=box))
    t["total_s"] = sum(t.values())
    return t, box, text


def driver_run(exe, tmp, cloud):
    src, dst = os.path.join(tmp, "cloud.bin"), os.path.join(tmp, "cloud.xyz")
    cloud.tofile(src)
    words = subprocess.run([exe, "cloud", src, dst, "filter"], check=True, capture_output=True, text=True).stdout.split()
    b = [int(w) for w in words[1:7]]
    t = {"bounds_s": float(words[10]), "text_s": float(words[11])}
    t["total_s"] = sum(t.values())
    return t, ((b[0], b[1]), (b[2], b[3]), (b[4], b[5])), open(dst, "rb").read()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--export-only", action="store_true", help="one export of the largest cloud on the device (for a kernel trace)")
    a = ap.parse_args()
    ctx = capi.Context(0)
    _, _, full = scene(max(SIZES))
    full = np.ascontiguousarray(full)
    if a.export_only:
        device_run(ctx, full[:1000])                            # (first use: module load, pool blocks)
        t, box, text = device_run(ctx, full)
        print("export: %d bytes, box %s, %s" % (len(text), box, {k: round(v * 1e3, 3) for k, v in t.items()}))
        return
    tmp = tempfile.mkdtemp(prefix="probe_xyz_export_")
    exe = os.path.join(tmp, "xyz_export_driver")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "xyz_export_driver.cpp")], check=True)
    out = {"device": ctx.device_info()["name"], "omp_threads": os.environ.get("OMP_NUM_THREADS"), "sizes": {}}
    device_run(ctx, full)                                       # (first use: module load, pool blocks, page-locked blocks)
    for n in SIZES:
        cloud = full[:n]
        rows = {"device": [], "device_from_points": [], "host_openmp": [], "driver_one_thread": []}
        points = capi.MeshPoints(ctx, cloud)
        equal = True
        for rep in range(3):
            td, box, text = device_run(ctx, cloud)
            tp, box_p, text_p = device_run(ctx, cloud, points=[points])
            th, box_h, text_h = host_run(cloud)
            tr, box_r, text_r = driver_run(exe, tmp, cloud)
            equal = equal and box == box_p == box_h == box_r and text == text_p == text_h == text_r
            for key, t in (("device", td), ("device_from_points", tp), ("host_openmp", th), ("driver_one_thread", tr)):
                rows[key].append(t)
        points.close()
        best = {k: min(r["total_s"] for r in v) for k, v in rows.items()}
        out["sizes"][str(n)] = {"bytes": len(text), "kept": text.count(b"\n"), "box": box, "all_equal": equal, "runs": rows, "best_total_s": best}
        print(n, "bytes", len(text), "equal", equal, {k: round(v * 1e3, 3) for k, v in best.items()}, flush=True)
        assert equal
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

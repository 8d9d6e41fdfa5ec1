"""Numbers, clouds and the yardstick program shared by test_xyz_export_host.py (the host route against the driver and
Python's '%g') and test_gpu_xyz_export.py (the device route against the host route).  Everything is compared byte for byte."""
import functools
import os
import subprocess
import tempfile

import numpy as np

from opencalibration_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOWEST, TWO63 = 1e-5, 2.0 ** 63   # the integer formatter covers 0 and LOWEST <= |v| < TWO63

EDGE_VALUES = [0.0, -0.0, 999999.5, 999999.49999999994, 99999.95, 0.0001, 9.9999949999e-5, 2.5e-5, 1e6, 1e15, 123456.5, 9.2e18,
               -999999.5, -99999.95, -2.5e-5, 1e-5, 100000.0, 1.0, -1.0, 0.5, 1234.5675, 2.0 ** 62, np.nextafter(TWO63, 0)]
FALLBACK_VALUES = [1e-7, 1e300, 5e-324, -5e-324, -1.7976931348623157e308, 2.0 ** 63, 2.0 ** 64, -1e-7, -1e300, 9.9999e-6, np.nextafter(LOWEST, 0)]


@functools.lru_cache(maxsize=None)
def driver():
    """The yardstick program, built once per process."""
    exe = os.path.join(tempfile.mkdtemp(prefix="xyz_export_driver_"), "xyz_export_driver")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "xyz_export_driver.cpp")],
                   check=True)
    return exe


def _scratch(name):
    return os.path.join(os.path.dirname(driver()), name)


def driver_format(values):
    """`ostream << v` of every value, as a list of bytes."""
    src, dst = _scratch("values.bin"), _scratch("values.txt")
    np.ascontiguousarray(values, np.float64).tofile(src)
    subprocess.run([driver(), "format", src, dst], check=True, timeout=120)
    lines = open(dst, "rb").read().split(b"\n")
    assert lines[-1] == b"" and len(lines) == len(values) + 1
    return lines[:-1]


def driver_cloud(xyz, bounds):
    """(box, kept, text) of the yardstick: bounds = "filter", None or three pairs."""
    src, dst = _scratch("cloud.bin"), _scratch("cloud.xyz")
    np.ascontiguousarray(xyz, np.float64).reshape(-1, 3).tofile(src)
    mode = ["filter"] if isinstance(bounds, str) else ["none"] if bounds is None else [str(int(v)) for pair in bounds for v in pair]
    r = subprocess.run([driver(), "cloud", src, dst, *mode], check=True, timeout=120, capture_output=True, text=True)
    words = r.stdout.split()
    assert words[0] == "bounds" and words[7] == "kept"
    b = [int(w) for w in words[1:7]]
    return ((b[0], b[1]), (b[2], b[3]), (b[4], b[5])), int(words[8]), open(dst, "rb").read()


def driver_obj(surfaces, geometry, name):
    """(obj, mtl) of the yardstick for surfaces given as (vertices, edges) arrays."""
    src, obj, mtl = _scratch("scene.txt"), _scratch("scene.obj"), _scratch("scene.mtl")
    w, h, min_x, max_y, gsd_x, gsd_y = geometry
    with open(src, "w") as f:
        f.write(f"{w} {h} {float(min_x).hex()} {float(max_y).hex()} {float(gsd_x).hex()} {float(gsd_y).hex()} {name}.mtl {name}.jpg "
                f"{len(surfaces)}\n")
        for v, e in surfaces:
            f.write(f"{len(v)} {len(e)}\n")
            for p in v:
                f.write(" ".join(float(c).hex() for c in p) + "\n")
            for row in e:
                f.write(" ".join(str(int(c)) for c in row) + "\n")
    subprocess.run([driver(), "obj", src, obj, mtl], check=True, timeout=120)
    return open(obj, "rb").read(), open(mtl, "rb").read()


@functools.lru_cache(maxsize=None)
def number_family():
    """More than 10^6 doubles the integer formatter covers: random bit patterns over its binades, uniform coordinates, the
    half-way cases (k + 0.5) / 10^j with both neighbours, multiples of half a unit of the sixth digit; and the edges."""
    rng = np.random.default_rng(2024)
    n = 260_000
    bits = (rng.integers(0, 1 << 52, n, dtype=np.uint64) | (rng.integers(1023 - 17, 1023 + 63, n, dtype=np.uint64) << np.uint64(52))
            | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63)))
    random_bits = bits.view(np.float64)
    uniform = rng.uniform(-2000, 2000, n)
    j = rng.integers(-3, 10, 100_000)
    k = rng.integers(0, 10 ** 6, 100_000)
    half = (k + 0.5) / 10.0 ** j
    halves = np.concatenate([half, np.nextafter(half, 0), np.nextafter(half, np.inf), -half])
    j = rng.integers(-4, 19, n)
    steps = rng.integers(2 * 10 ** 5, 2 * 10 ** 6, n)                  # six digits and a half: 100000.0, 100000.5, ...
    sixth = steps * 0.5 * 10.0 ** j / 10 ** 6
    v = np.concatenate([random_bits, uniform, halves, sixth, -sixth[:50_000], EDGE_VALUES])
    v = v[(v == 0) | ((np.abs(v) >= LOWEST) & (np.abs(v) < TWO63))]
    assert len(v) > 10 ** 6
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def number_family_text():
    """The yardstick's text of number_family() as an S16 array (computed once)."""
    return np.array(driver_format(number_family()), dtype="S16")


def survey_cloud(n=5000, outliers=40, seed=3):
    rng = np.random.default_rng(seed)
    body = np.column_stack([rng.uniform(-120, 120, n), rng.uniform(-120, 120, n), rng.normal(-48, 1.5, n)])
    far = rng.normal(0, 400, (outliers, 3))
    pts = np.concatenate([body, far])
    return pts[rng.permutation(len(pts))]


@functools.lru_cache(maxsize=None)
def cloud_cases():
    """name -> per surface its list of clouds."""
    rng = np.random.default_rng(17)
    line = lambda n: np.column_stack([np.linspace(-30.3, 41.7, n), np.linspace(5.2, 93.9, n), np.linspace(-3.4, 7.7, n)])
    survey = survey_cloud()
    cases = {
        "empty": [[]],
        "one_point": [[np.array([[12.25, -7.5, 103.0625]])]],
        "one_cell": [[rng.uniform(3.1, 3.9, (50, 3))]],
        "flat_z": [[np.column_stack([rng.uniform(-40, 40, 300), rng.uniform(-40, 40, 300), rng.uniform(5.2, 5.8, 300)])]],
        "n39": [[line(39)]],
        "n40": [[line(40)]],
        "straddle_zero": [[np.concatenate([rng.uniform(-0.9, 0.9, (60, 3)), rng.uniform(-3.5, 3.5, (200, 3)),
                                            [[-0.9, 0.9, -0.0], [0.9, -0.9, 0.0]]])]],
        "survey": [[survey]],
        "far_point": [[np.concatenate([survey[:300], [[1e12, 3.0, -48.0]], survey[300:600]])]],
        "two_by_two": [[survey[:700], survey[700:1500]], [survey[1500:1900], survey[1900:2600]]],
    }
    return cases


def flat(case):
    parts = [c for clouds in case for c in clouds]
    return np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, 3)))


def surfaces_of(case):
    return [host.Surface().set_clouds(list(clouds)) for clouds in case]


CUSTOM_BOX = ((-100, 57), (-33, 120), (-50, -46))

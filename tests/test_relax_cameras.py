"""What the relax set-ups share on the host (csrc/host/relax_cameras.hpp): the camera table of nodeid2poseopt, the
bootstrap plane and the packing of plane edges, under the sanitizers in a stand-alone program that links no device
library and loads nothing into Python."""
import functools
import os
import subprocess
import tempfile
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(None)
def driver():
    """tests/relax_cameras_driver.cpp built with the address and undefined-behaviour sanitizers; without where the
    runtime does not link.  Returns (path, sanitized)."""
    exe = os.path.join(tempfile.mkdtemp(prefix="relax_cameras_driver_"), "relax_cameras_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fopenmp", "-o", exe,
           os.path.join(ROOT, "tests", "relax_cameras_driver.cpp")]
    if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode == 0:
        return exe, True
    subprocess.run(cmd, check=True)
    return exe, False


def test_camera_table_plane_and_packer_in_a_standalone_program():
    """An empty pose list; poses [7, 9, 7] (cameras 0 and 1, the later pose of 7 untouched by the normalising write-back);
    an optimised pose without an orientation; context cameras in the order 4, 2, 4 and three nodes that give none; the
    plane over three positions and over one; two lens models over three edges, cumulative inlier offsets and the
    descriptor score of an inlier that names no match: the program checks its own answers and ends clean"""
    exe, sanitized = driver()
    if not sanitized:
        warnings.warn("the address,undefined sanitizer runtime does not link here: the stand-alone program ran without -fsanitize")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, OMP_NUM_THREADS="4"))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]

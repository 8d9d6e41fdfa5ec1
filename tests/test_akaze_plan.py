"""AKAZE's schedule as data (csrc/akaze_plan.hpp): the level table, the FED groups, the form of every launch and the planes
it reads and writes, walked under the sanitizers in a stand-alone program that links no device library and loads nothing
into Python."""
import functools
import os
import subprocess
import tempfile
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(None)
def driver():
    """tests/akaze_plan_driver.cpp built with the address and undefined-behaviour sanitizers; without where the runtime
    does not link.  Returns (path, sanitized)."""
    exe = os.path.join(tempfile.mkdtemp(prefix="akaze_plan_driver_"), "akaze_plan_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "akaze_plan_driver.cpp")]
    if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode == 0:
        return exe, True
    subprocess.run(cmd, check=True)
    return exe, False


def test_plans_of_seven_calls_executed_symbolically_in_a_standalone_program():
    """The bench chunk (1600 x 1200 x 100), the planes test's mixed route (640 x 320, threshold 320 * 160), 640 x 480 under
    tile_levels,tile_det and under strip_levels,strip_det, 501 x 334 (odd sizes: tiles, the area half-sample), 640 x 200
    (three octaves) and 72 x 48 (one).  Every plane holds a tag and every launch checks the tag it reads: each level's
    last launch leaves "level i after all its steps" in Lt[i], no launch reads and writes one plane, an image half-sampled
    by a strip epilogue is what the next level's first launch reads and no half-sample launch is planned there, the groups
    sum to the step count with each <= FED_FUSE, every planned (sigma_size, K, store_flow) is instantiated, the per-level
    table is 2 3 3 4 per octave and 3 3 4 | 4 5 6 7 | 8 10 12 14 | 17 20 24 29 steps, and the routes are the expected
    ones: the program checks its own answers and ends clean"""
    exe, sanitized = driver()
    if not sanitized:
        warnings.warn("the address,undefined sanitizer runtime does not link here: the stand-alone program ran without -fsanitize")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:] + r.stderr[-4000:]

"""The hand-over of the extraction contexts between surveys (csrc/host/extract_slots.hpp), without a device: a small
program (tests/extract_slots_driver.cpp) runs surveys as threads through the protocol extract_features_stream follows, with
sleeps for the device and the host tail, built with the system g++ - under the thread sanitizer where the toolchain links
it (host code only).  It checks, in seeded random schedules of 2 - 4 surveys x 1 - 13 chunks x 1 - 5 slots with random chunk
durations and one survey failing half-way: never two holders of a slot, chunks handed out in ticket order, never more
chunks in flight than slots, no buffer with two users, every schedule ends (the time limit below); and in the 10-chunk /
4-slot case that a slot freed by survey k runs survey k + 1 before survey k's last chunk has finished."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "extract_slots_driver.cpp")


def _links_tsan(tmp):
    probe = os.path.join(tmp, "probe.cpp")
    with open(probe, "w") as f:
        f.write("#include <thread>\nint main() { std::thread t([] {}); t.join(); return 0; }\n")
    exe = os.path.join(tmp, "probe")
    r = subprocess.run(["g++", "-std=c++17", "-pthread", "-fsanitize=thread", "-o", exe, probe], capture_output=True)
    if r.returncode != 0:
        return False
    # (a sanitizer runtime that links but cannot map its shadow memory in this process's address space is no use either)
    return subprocess.run([exe], capture_output=True, timeout=60).returncode == 0


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("extract_slots"))
    exe = os.path.join(tmp, "extract_slots_driver")
    flags = ["-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Wextra"]
    tsan = _links_tsan(tmp)
    if tsan:
        flags.append("-fsanitize=thread")
    subprocess.run(["g++", *flags, "-o", exe, SRC], check=True)
    print("thread sanitizer:", "on" if tsan else "not available")
    return exe


def _run(exe, *args):
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=240, env=env)
    print(r.stdout[-2000:])
    print(r.stderr[-4000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert "FAIL" not in r.stdout and "ThreadSanitizer" not in r.stderr
    return r.stdout


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_schedules_keep_the_invariants(driver, seed):
    out = _run(driver, "random", str(seed), "60")
    assert out.strip().splitlines()[-1].startswith("ok 60 schedules")


def test_next_survey_runs_on_a_freed_slot_before_the_last_chunk_finishes(driver):
    out = _run(driver, "handover")
    assert out.strip().splitlines()[-1] == "ok handover"
